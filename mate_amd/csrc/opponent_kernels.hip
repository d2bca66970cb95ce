// opponent_kernels.hip -- the opponents' kernels beyond the Greedy pair, both teams' (opponent_rows.hpp), as a translation unit of its own: their
// kernel-resource remarks are kept apart from the other units' (mate_amd/build.py: lib/kernel_resources_opponents.json).
#include <hip/hip_runtime.h>
#include "opponent_kernels.inc"
