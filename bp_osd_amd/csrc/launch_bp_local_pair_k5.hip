// launch_bp_local_pair_k5.hip -- bp_local_kernel instances with a loop body for the wave (group key 5, mixed group)
#define BPL_PAIRKEY 5
#include "launch_bp_local_pair.inc.h"
