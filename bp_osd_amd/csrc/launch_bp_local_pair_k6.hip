// launch_bp_local_pair_k6.hip -- bp_local_kernel instances with a loop body for the wave (group key 6, mixed group)
#define BPL_PAIRKEY 6
#include "launch_bp_local_pair.inc.h"
