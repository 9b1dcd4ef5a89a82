// launch_bp_local_pair_k10.hip -- bp_local_kernel instances with a loop body for the wave (group key 10, mixed group)
#define BPL_PAIRKEY 10
#include "launch_bp_local_pair.inc.h"
