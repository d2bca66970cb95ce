// shape_group.inc -- the kernels of ONE group of scenario shapes (shape_groups.hpp), selected by MATE_SHAPE_GROUP: compiled as a
// translation unit of its own through shape_group.hip, or included by mate_engine.hip once per group in a single-unit build.
#if MATE_SHAPE_GROUP == 0
#define MATE_GROUP_SHAPES MATE_SHAPES_G0
#define MATE_GROUP_FN pick_kernels_group0
#elif MATE_SHAPE_GROUP == 1
#define MATE_GROUP_SHAPES MATE_SHAPES_G1
#define MATE_GROUP_FN pick_kernels_group1
#elif MATE_SHAPE_GROUP == 2
#define MATE_GROUP_SHAPES MATE_SHAPES_G2
#define MATE_GROUP_FN pick_kernels_group2
#elif MATE_SHAPE_GROUP == 3
#define MATE_GROUP_SHAPES MATE_SHAPES_G3
#define MATE_GROUP_FN pick_kernels_group3
#elif MATE_SHAPE_GROUP == 4
#define MATE_GROUP_SHAPES MATE_SHAPES_G4
#define MATE_GROUP_FN pick_kernels_group4
#else
#define MATE_GROUP_SHAPES MATE_SHAPES_G5
#define MATE_GROUP_FN pick_kernels_group5
#endif

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
#undef MATE_GROUP_SHAPES
#undef MATE_GROUP_FN
