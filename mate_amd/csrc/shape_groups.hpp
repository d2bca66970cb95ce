// shape_groups.hpp -- the scenario shapes (cameras, targets, obstacles) with compiled specialisations of the kernels: EVERY scenario
// the reference ships (mate/assets/MATE-{1v1,1v2,2v2,2v4,4v2,4v4,4v8,8v8}-{0,9}.yaml, MATE-Navigation.yaml; MATE.yaml = 4v8-9).  A
// generic (AnyShape) fused rollout runs at less than half the rate of a specialised one (MATE-4v8-9 x 4096: 2.8e8 against 6.4e8
// env-steps/s), so until round 4 twelve of the seventeen shipped scenarios ran at half speed.  The shapes are compiled in six
// groups -- six translation units built in parallel by mate_amd/build.py (one unit with all of them takes four minutes).
// X: all kernels, f32 and f64 observations (the five shapes of BASELINE.json's configurations and the parity traces);
// Y: f32 observations only -- an f64-observation engine of such a shape runs the generic kernels.
#pragma once
#include <type_traits>

#include "policy_kernels.hpp"

namespace mate {

using StepFn = void (*)(const Params *, const Ptrs);
using PolicyFn = void (*)(const Params *, const Ptrs, const PolicyPtrs);

#define MATE_SHAPES_G0(X, Y) X(4, 8, 9) X(4, 8, 0)
#define MATE_SHAPES_G1(X, Y) X(8, 8, 9) Y(8, 8, 0)
#define MATE_SHAPES_G2(X, Y) X(4, 2, 9) X(0, 8, 32) Y(4, 2, 0)
#define MATE_SHAPES_G3(X, Y) Y(4, 4, 9) Y(4, 4, 0) Y(2, 4, 9)
#define MATE_SHAPES_G4(X, Y) Y(2, 4, 0) Y(2, 2, 9) Y(2, 2, 0)
#define MATE_SHAPES_G5(X, Y) Y(1, 2, 9) Y(1, 2, 0) Y(1, 1, 9) Y(1, 1, 0)

// One default: no split form, no row image, no sub-wave kernels, one environment per wave.  Everything that fills a set starts here.
struct KernelSet {
    StepFn step[3] = {};               // [flow]
    StepFn split[3] = {};              // step_split_kernel per flow (two waves per environment), or null
    StepFn rollout[2] = {};            // [0] generic flow, [1] FLOW_RANDOM (the row-image compilation where the shape has one and `image` says so)
    PolicyFn policy = nullptr, rollout_greedy = nullptr;
    PolicyFn step_greedy = nullptr;    // step_greedy_kernel: the per-step flows with the on-device agents as ONE launch (f32 observations), or null
    int image = 0;
    // E environments per wave (FixedShape::kSubWave, f32 observations): the fused rollouts of the small scenarios, or null / 1
    StepFn rollout_sub[3] = {};        // [flow]: FLOW_ANY, FLOW_RANDOM, FLOW_ACT_F32 (the one-step form behind mate_engine_step)
    PolicyFn rollout_greedy_sub = nullptr;
    int sub_wave = 1;
    int specialised = 0;               // compiled for the scenario's shape (pick_kernels: a shape group filled the set), not the generic (AnyShape) kernels
};

// The kernels of one shape policy.  f32 observations, the product path: a kernel per launch-flag specialisation (enum Flow), the
// two-wave step of the folded flows, and where they exist the sub-wave rollouts (Shape::kSubWave environments per wave), the
// one-launch Greedy step (`kStepGreedy`: step_greedy_compiled) and the row-image rollout (`ImageShape`; void: the shape has none).
template <class Shape, class ImageShape, bool kStepGreedy>
KernelSet f32_kernels(bool no_image) {
    KernelSet k;
    k.step[FLOW_ANY] = (StepFn)step_kernel<float, Shape>;
    k.step[FLOW_RANDOM] = (StepFn)step_kernel<float, Shape, FLOW_RANDOM>;
    k.step[FLOW_ACT_F32] = (StepFn)step_kernel<float, Shape, FLOW_ACT_F32>;
    k.split[FLOW_RANDOM] = (StepFn)step_split_kernel<float, Shape, FLOW_RANDOM>;
    k.split[FLOW_ACT_F32] = (StepFn)step_split_kernel<float, Shape, FLOW_ACT_F32>;
    k.rollout[0] = (StepFn)rollout_kernel<float, Shape>;
    k.rollout[1] = (StepFn)rollout_kernel<float, Shape, FLOW_RANDOM>;
    k.policy = (PolicyFn)greedy_policy_kernel<float, Shape>;
    k.rollout_greedy = (PolicyFn)rollout_greedy_kernel<float, Shape>;
    if constexpr (kStepGreedy) k.step_greedy = (PolicyFn)step_greedy_kernel<float, Shape>;
    if constexpr (Shape::kSubWave > 1) {
        constexpr int E = Shape::kSubWave;
        k.rollout_sub[0] = (StepFn)rollout_kernel<float, Shape, FLOW_ANY, E>;
        k.rollout_sub[1] = (StepFn)rollout_kernel<float, Shape, FLOW_RANDOM, E>;
        k.rollout_sub[2] = (StepFn)rollout_kernel<float, Shape, FLOW_ACT_F32, E>;
        k.rollout_greedy_sub = (PolicyFn)rollout_greedy_kernel<float, Shape, E>;
        k.sub_wave = E;
    }
    if constexpr (!std::is_void_v<ImageShape>) {
        if (!no_image) { k.rollout[1] = (StepFn)rollout_kernel<float, ImageShape, FLOW_RANDOM>; k.image = 1; }
    }
    (void)no_image;
    return k;
}
// f64 observations, the parity mirror: the generic flow everywhere, the two-launch form of the Greedy step.
template <class Shape>
KernelSet f64_kernels() {
    KernelSet k;
    k.step[FLOW_ANY] = k.step[FLOW_RANDOM] = k.step[FLOW_ACT_F32] = (StepFn)step_kernel<double, Shape>;
    k.rollout[0] = k.rollout[1] = (StepFn)rollout_kernel<double, Shape>;
    k.policy = (PolicyFn)greedy_policy_kernel<double, Shape>;
    k.rollout_greedy = (PolicyFn)rollout_greedy_kernel<double, Shape>;
    return k;
}
// (a compiled scenario shape: its row-image form and its step_greedy_kernel exist where image_fits / step_greedy_compiled say so)
template <int C, int T, int O>
KernelSet fixed_f32_kernels(bool no_image) {
    return f32_kernels<FixedShape<C, T, O, false>, std::conditional_t<image_fits(C, T, O), FixedShape<C, T, O, false, true>, void>, step_greedy_compiled(C, T, O)>(no_image);
}

// true = the group holds the shape and `out` is filled (false for an f64-observation engine of a Y shape)
bool pick_kernels_group0(int Nc, int Nt, int No, bool f64, bool no_image, KernelSet *out);
bool pick_kernels_group1(int Nc, int Nt, int No, bool f64, bool no_image, KernelSet *out);
bool pick_kernels_group2(int Nc, int Nt, int No, bool f64, bool no_image, KernelSet *out);
bool pick_kernels_group3(int Nc, int Nt, int No, bool f64, bool no_image, KernelSet *out);
bool pick_kernels_group4(int Nc, int Nt, int No, bool f64, bool no_image, KernelSet *out);
bool pick_kernels_group5(int Nc, int Nt, int No, bool f64, bool no_image, KernelSet *out);

}  // namespace mate
