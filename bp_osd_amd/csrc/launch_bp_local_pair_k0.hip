// launch_bp_local_pair_k0.hip -- bp_local_kernel instances with a loop body for the wave (group key 0, mixed group)
#define BPL_PAIRKEY 0
#include "launch_bp_local_pair.inc.h"
