// launch_bp_local_pair_k1.hip -- bp_local_kernel instances with a loop body for the wave (group key 1, mixed group)
#define BPL_PAIRKEY 1
#include "launch_bp_local_pair.inc.h"
