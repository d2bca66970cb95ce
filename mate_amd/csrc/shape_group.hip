// shape_group.hip -- the kernels of ONE group of scenario shapes (shape_groups.hpp: MATE_SHAPES_G<k>, pick_kernels_group<k>) as a translation
// unit of its own, selected by -DMATE_SHAPE_GROUP=k; mate_amd/build.py compiles one unit per group, in parallel.
#include <hip/hip_runtime.h>
#include "shape_groups.hpp"

#ifndef MATE_SHAPE_GROUP
#error "shape_group.hip: compile with -DMATE_SHAPE_GROUP=k, one of the groups of shape_groups.hpp"
#endif
#define MATE_PASTE_(a, b) a##b
#define MATE_PASTE(a, b) MATE_PASTE_(a, b)      // (through a second macro: MATE_SHAPE_GROUP is expanded to its number first)
#define MATE_GROUP_SHAPES MATE_PASTE(MATE_SHAPES_G, MATE_SHAPE_GROUP)
#define MATE_GROUP_FN MATE_PASTE(pick_kernels_group, MATE_SHAPE_GROUP)

namespace mate {

bool MATE_GROUP_FN(int Nc, int Nt, int No, bool f64, bool no_image, KernelSet *out) {
#define X(C, T, O) if (Nc == C && Nt == T && No == O) { *out = f64 ? f64_kernels<FixedShape<C, T, O, true>>() : fixed_f32_kernels<C, T, O>(no_image); return true; }
#define Y(C, T, O) if (Nc == C && Nt == T && No == O) { if (f64) return false; *out = fixed_f32_kernels<C, T, O>(no_image); return true; }
    MATE_GROUP_SHAPES(X, Y)
#undef X
#undef Y
    return false;
}

}  // namespace mate
