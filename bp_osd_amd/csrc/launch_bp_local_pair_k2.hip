// launch_bp_local_pair_k2.hip -- bp_local_kernel instances with a loop body for the wave (group key 2, mixed group)
#define BPL_PAIRKEY 2
#include "launch_bp_local_pair.inc.h"
