// render_rows.hpp -- render_kernel: MultiAgentTracking.render(mode='rgb_array') (environment.py:986-1180 of the reference) rasterised on the device, the
// rules of DESIGN.md 3.20.  Not on the step path: ONE launch on demand (mate_engine_render) over the records and the engine's own mask words as the last call
// left them; it writes the caller's frames and nothing else.
//
// The picture is the reference's display list in its order, point-sampled at the pixel centres of the view [-1050, 1050]^2, row 0 at the top, on white:
//   0            the margin: the closed polyline of the terrain's square, width 3
//   1 .. 4       the warehouses' base squares (alpha 0.6, or 0.3 once nothing remains and nothing waits there; the PNG icons are not drawn)
//   5 ..         the obstacles: regular 72-gons
//   per camera   the sector under the knots at sight_range (0, .6, .8, .1), then the field-of-view polygon under the knots' own rhos clipped to
//                [radius, sight_range] (green where the camera sees a target, else yellow; alpha .25): ONE slot, two blends
//   per camera   the base 72-gon (perceived / unperceived), the body and the lens quads, all three turned by the orientation
//   per target   the tracked marker (a 15-gon), where tracked
//   per target   the arrow (capacity 1: six vertices, else five; fans from vertex 0) in its goal's colour, turned by its heading; then, loaded without a bounty,
//                the same at scale 0.4 in white, alpha .66
// With a communication trace (trace_rows.hpp) RenderCommunication's arrows go where its callback prepends them to the one-time list: behind the
// obstacles, ahead of the first camera's sector.  Cameras' pairs then targets', sender-major, every pair with remaining > 0 and distinct positions: draw_arrow's two
// or three lines (render_communication.py:66-92), each a dashed segment of width 2.5 pixels -- a centre is covered within 1.25 pitches of the segment and where
// floor(u) mod 8 < 4, u the distance of its clamped projection from the line's FIRST vertex along the segment's major axis in pitches (stipple 0x0F0F, factor 1).
// The workgroup keeps the pairs whose endpoints' box, padded by 60 + 1.25 pitches, meets the tile (the same ordered compaction), builds their lines in LDS
// kRenderArrowChunk pairs at a time at that list position, and every pixel walks them.
// A primitive blends ONCE per pixel, dst = src a + dst (1 - a) in f32 without contraction, and the pixel is quantised once, floor(255 c + 0.5).
//
// Mapping: one 256-thread workgroup per 16 x 16 pixel tile of one requested environment, thread = pixel.  The workgroup first writes the environment's
// display list into LDS as records of kRenderPrimWords doubles (one thread per slot: vertices in world coordinates, bounding box, colour), keeps the slots whose
// box meets the tile's (an ordered compaction: the test is the same for every lane, a tile pays for what can touch it), and every pixel walks that list.
// Geometry in f64.  The field of view needs no vertex list: the fan from the camera over the knots of boundary_between is star-shaped, so the pixel's bearing
// finds its wedge in the camera's table (the bucket table, then a short search), the wedge's two knots -- or the sector's ends, interpolated once per workgroup --
// give one far edge and ONE cross product decides; the flanks are two more against the ends' directions.  The 72-gons and 15-gons are decided by their
// circumscribed and inscribed circles except in the thin ring between the two, where the edges are walked.
// The frame leaves as 16-byte pieces from an LDS image of the tile where the size is a multiple of 16 (every row of every tile then starts on a 16-byte boundary
// of a 16-byte aligned buffer), pixel by pixel otherwise.  Offsets are 64-bit.
//
// This header holds the arguments, the kernel template and the launch function's declaration; render_kernels.hip instantiates it, a translation unit of its own.
#pragma once
#include "engine_kernels.hpp"

namespace mate {

constexpr int kRenderTile = 16;                       // pixels per side of a workgroup's tile
constexpr int kRenderMinSize = 16, kRenderMaxSize = 4096;
constexpr int kRenderPrimWords = 22;                  // doubles per slot: 12 vertex words | box x0 x1 y0 y1 | half width, - | rgba (4 f32) | kind, vertices, camera, pad (4 i32)
constexpr int kRenderCamWords = 12;                   // doubles per camera: x y | left theta | sight radius | rho_left rho_right (clipped) | cos sin left | cos sin right
constexpr int kRenderMaxSlots = 256;                  // 5 + No + 4 Nc + 3 Nt <= 181 for every shape the engine takes
constexpr double kRenderBound = 1.05 * kTerrain;      // environment.py:1017
constexpr double kTargetRenderRadius = 27.5;          // environment.py:42
enum RenderKind : int32_t { RENDER_NONE = 0, RENDER_FAN = 1, RENDER_NGON = 2, RENDER_VIEW = 3, RENDER_LOOP = 4 };

struct RenderArgs {
    const double *stat, *dyn;                         // Ptrs::stat, Ptrs::dyn
    const double2 *knots; const uint16_t *bucket; const int32_t *knot_count;      // Ptrs::lut_knots, lut_bucket, lut_count
    const uint32_t *masks;                            // Ptrs::own_masks
    const int32_t *envs;                              // [count] environments to draw, any order, repeats allowed; null: 0 .. count - 1
    const double *headings;                           // [count][Nt] target_orientations in degrees; null: zeros
    uint8_t *out;                                     // [count][size][size][3]
    int64_t N;
    int32_t count, size, bit_ct, bit_tr;
    const uint8_t *trace[2];                          // the teams' remaining[N][n][n] of the communication trace (trace_rows.hpp), or null
    const int32_t *trace_tags[2];                     // [N] the episode number each matrix belongs to
    int32_t duration;                                 // of the trace; 0: no arrows, and nothing below is read
};

__host__ __device__ constexpr int render_slots(int Nc, int Nt, int No) { return 5 + No + 4 * Nc + 3 * Nt; }
// dynamic LDS, every part a multiple of 16 bytes: the slots, the cameras, the polygons' unit vertices (72 + 15 pairs), the tile's list, the tile's image, the flags
constexpr int kRenderImageBytes = kRenderTile * kRenderTile * 3, kRenderFlagWords = 24;      // flags: 16 cameras | tracked | 4 wave counts | pad
__host__ __device__ constexpr int render_lds_bytes(int Nc, int Nt, int No) {
    return (render_slots(Nc, Nt, No) * kRenderPrimWords + (Nc > 0 ? Nc : 1) * kRenderCamWords + 2 * (72 + 15)) * 8 + kRenderMaxSlots * 2 + kRenderImageBytes + kRenderFlagWords * 4;
}

// the arrows' part, behind everything above and only in a launch with a trace: the lines of a chunk of pairs, the listed pairs, 4 wave counts
constexpr int kRenderArrowChunk = 128, kRenderArrowWords = 9, kRenderMaxPairs = 512;      // doubles per pair: start | end | end - vec1 | end - vec2 | alpha (f32), lines (i32)
constexpr int kRenderArrowBytes = kRenderArrowChunk * kRenderArrowWords * 8 + kRenderMaxPairs * 2 + 16;
constexpr double kArrowHead = 0.05 * kTerrain, kArrowOffset = 0.01 * kTerrain, kArrowHalfWidth = 1.25;      // render_communication.py:71-80; half of stroke 2.5, in pitches

__device__ __forceinline__ double render_cross(double ax, double ay, double bx, double by) { return ax * by - ay * bx; }

// np.interp on a camera's knots at `x` in [-180, 180): Camera.sight_range_at (lut_lookup's arithmetic; a full search: once per camera and workgroup)
__device__ __forceinline__ double render_interp(const double2 *knots, int n, double x) {
    int lo = 0, hi = n - 1;
    while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (knots[mid].x <= x) lo = mid; else hi = mid; }
    if (knots[hi].x <= x) lo = hi;
    const double2 k0 = knots[lo];
    if (lo >= n - 1 || k0.x == x) return k0.y;
    const double2 k1 = knots[lo + 1];
    const double slope = (k1.y - k0.y) / (k1.x - k0.x);
    double res = slope * (x - k0.x) + k0.y;
    if (res != res) {
        res = slope * (x - k1.x) + k1.y;
        if (res != res && k0.y == k1.y) res = k0.y;
    }
    return res;
}

// the pixel is inside the fan triangle (a, b, c), either orientation, edges included
__device__ __forceinline__ bool render_in_triangle(double px, double py, double ax, double ay, double bx, double by, double cx, double cy) {
    const double c1 = render_cross(bx - ax, by - ay, px - ax, py - ay);
    const double c2 = render_cross(cx - bx, cy - by, px - bx, py - by);
    const double c3 = render_cross(ax - cx, ay - cy, px - cx, py - cy);
    return (c1 >= 0.0 && c2 >= 0.0 && c3 >= 0.0) || (c1 <= 0.0 && c2 <= 0.0 && c3 <= 0.0);
}

__device__ __forceinline__ float render_blend(float dst, float src, float a) { return __fadd_rn(__fmul_rn(src, a), __fmul_rn(dst, __fsub_rn(1.0f, a))); }
__device__ __forceinline__ uint32_t render_quantise(float c) {
    const float q = __builtin_floorf(__fadd_rn(__fmul_rn(255.0f, c), 0.5f));
    return (uint32_t)(q < 0.0f ? 0.0f : (q > 255.0f ? 255.0f : q));
}

// One dashed line a -> b at the pixel centre (px, py): within `half` of the segment, and in an on-phase of the stipple counted from a
__device__ __forceinline__ bool render_dash(double px, double py, double ax, double ay, double bx, double by, double half, double pitch) {
    const double ex = bx - ax, ey = by - ay;
    const double t = clipd(((px - ax) * ex + (py - ay) * ey) / (ex * ex + ey * ey), 0.0, 1.0);
    const double qx = t * ex, qy = t * ey;
    const double ox = px - (ax + qx), oy = py - (ay + qy);
    if (!(ox * ox + oy * oy <= half * half)) return false;
    const double along = __builtin_fabs(ex) >= __builtin_fabs(ey) ? __builtin_fabs(qx) : __builtin_fabs(qy);
    return ((int)floor(along / pitch) & 7) < 4;
}

// `kWide`: the size is a multiple of 16 -- the tile's rows leave as 16-byte pieces
template <bool kWide>
__global__ __launch_bounds__(256, 4) void render_kernel(const Params *__restrict__ pp, const RenderArgs a) {
    extern __shared__ __align__(16) unsigned char render_lds[];
    const Params &p = *pp;
    const int Nc = p.Nc, Nt = p.Nt, No = p.No;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int S = a.size, T = (S + kRenderTile - 1) / kRenderTile;
    const int k = (int)(blockIdx.x / (unsigned)(T * T)), tile = (int)(blockIdx.x % (unsigned)(T * T));
    if (k >= a.count) return;
    const int64_t env = a.envs ? (int64_t)a.envs[k] : (int64_t)k;
    if (env < 0 || env >= a.N) return;                // (the same in every lane: the frame stays as it is)
    const int ty = tile / T, tx = tile - ty * T;
    const int slots = render_slots(Nc, Nt, No);
    double *prims = reinterpret_cast<double *>(render_lds);
    double *cams = prims + slots * kRenderPrimWords;
    double *unit = cams + (Nc > 0 ? Nc : 1) * kRenderCamWords;      // (cos, sin) of 5 i degrees, i < 72, then of 24 i degrees, i < 15
    uint16_t *list = reinterpret_cast<uint16_t *>(unit + 2 * (72 + 15));
    uint8_t *image = reinterpret_cast<uint8_t *>(list + kRenderMaxSlots);
    uint32_t *cam_flags = reinterpret_cast<uint32_t *>(image + kRenderImageBytes);      // bit 0: the camera sees a target; bit 1: a target perceives it
    uint32_t *tracked_bits = cam_flags + 16, *wave_hits = cam_flags + 17;
    const double *st = a.stat + env * p.SW, *dy = a.dyn + env * p.DW;
    const int32_t *di = reinterpret_cast<const int32_t *>(dy + p.DF);
    const uint32_t *mw = a.masks + env * p.MW;

    // ---------------------------------------------------------------------------------------------- 0: unit polygons, mask bits, cameras
    if (tid < 72 + 15) {
        double sn, cs;
        sincos_deg(tid < 72 ? 5.0 * (double)tid : 24.0 * (double)(tid - 72), sn, cs);
        unit[2 * tid] = cs; unit[2 * tid + 1] = sn;
    } else if (tid >= 96 && tid < 96 + Nc) {
        const int c = tid - 96;
        uint32_t sees = 0u, perceived = 0u;
        for (int t = 0; t < Nt; ++t) {
            const int b0 = a.bit_ct + c * Nt + t, b1 = a.bit_tr + t * p.NJ + c;
            sees |= (mw[b0 >> 5] >> (b0 & 31)) & 1u;
            perceived |= (mw[b1 >> 5] >> (b1 & 31)) & 1u;
        }
        cam_flags[c] = sees | (perceived << 1);
    } else if (tid == 128) {
        uint32_t tracked = 0u;
        for (int t = 0; t < Nt; ++t)
            for (int c = 0; c < Nc; ++c) {
                const int b0 = a.bit_ct + c * Nt + t;
                tracked |= ((mw[b0 >> 5] >> (b0 & 31)) & 1u) << t;
            }
        *tracked_bits = tracked;
    } else if (tid >= 192 && tid < 192 + Nc) {
        const int c = tid - 192;
        const int64_t item = env * Nc + c;
        const double phi = dy[c], theta = dy[Nc + c];
        const double sight = sqrt_pos(div_nz(p.area, theta)), half = theta / 2.0;
        const double left = normalize_angle(phi - half);                     // entities.py:516-519
        const double right = left + ((phi + half) - (phi - half));
        const double2 *kn = a.knots + item * p.kmax;
        int n = a.knot_count[item];
        n = n > p.kmax ? p.kmax : n;
        double rho_l = sight, rho_r = sight;                                 // (a table of fewer than two knots was never built: the view slot draws nothing)
        if (n >= 2) { rho_l = render_interp(kn, n, left); rho_r = render_interp(kn, n, normalize_angle(right)); }
        double *cr = cams + c * kRenderCamWords;
        cr[0] = st[c]; cr[1] = st[Nc + c]; cr[2] = left; cr[3] = right - left; cr[4] = sight; cr[5] = p.cam_radius;
        cr[6] = clipd(rho_l, p.cam_radius, sight); cr[7] = clipd(rho_r, p.cam_radius, sight);
        double sn, cs;
        sincos_deg(left, sn, cs); cr[8] = cs; cr[9] = sn;
        sincos_deg(right, sn, cs); cr[10] = cs; cr[11] = sn;
    }
    __syncthreads();

    // ---------------------------------------------------------------------------------------------- 1: the display list, one thread per slot
    if (tid < slots) {
        double *q = prims + tid * kRenderPrimWords;
        float *rgba = reinterpret_cast<float *>(q + 18);
        int32_t *meta = reinterpret_cast<int32_t *>(q + 20);
        int kind = RENDER_NONE, nv = 0, aux = 0;
        float cr = 0.f, cg = 0.f, cb = 0.f, ca = 1.f;
        double x0 = 0.0, x1 = 0.0, y0 = 0.0, y1 = 0.0;                       // the box
        // a polygon given by unit vertices (ux, uy), scaled, turned by (cs, sn), moved to (ox, oy): Transform.enable's order (pygletrendering.py:227-231)
        auto put = [&](int i, double ux, double uy, double scale, double cs, double sn, double ox, double oy) {
            const double sx = scale * ux, sy = scale * uy;
            const double vx = ox + (cs * sx - sn * sy), vy = oy + (sn * sx + cs * sy);
            q[2 * i] = vx; q[2 * i + 1] = vy;
            if (i == 0) { x0 = x1 = vx; y0 = y1 = vy; }
            x0 = vx < x0 ? vx : x0; x1 = vx > x1 ? vx : x1; y0 = vy < y0 ? vy : y0; y1 = vy > y1 ? vy : y1;
        };
        const int base_view = 5 + No, base_cam = base_view + Nc, base_marker = base_cam + 3 * Nc, base_target = base_marker + Nt;
        if (tid == 0) {                                                      // margin (environment.py:1034-1038), default colour: black
            kind = RENDER_LOOP; nv = 4;
            put(0, 1.0, 1.0, kTerrain, 1.0, 0.0, 0.0, 0.0); put(1, -1.0, 1.0, kTerrain, 1.0, 0.0, 0.0, 0.0);
            put(2, -1.0, -1.0, kTerrain, 1.0, 0.0, 0.0, 0.0); put(3, 1.0, -1.0, kTerrain, 1.0, 0.0, 0.0, 0.0);
            const double grow = 1.5 * (2.0 * kRenderBound / (double)S);
            q[16] = grow;                                                    // (half the width in world units)
            x0 -= grow; x1 += grow; y0 -= grow; y1 += grow;
        } else if (tid < 5) {                                                // warehouses (environment.py:1041-1053, 1118-1126)
            const int w = tid - 1;
            const int32_t *ei = di + Nt * TI_STRIDE;
            const int32_t *r = ei + EI_REMAINING + 4 * w;
            const bool busy = r[0] + r[1] + r[2] + r[3] > 0 || ei[EI_AWAITING + w] > 0;
            const double wx = (w == 1 || w == 2) ? -kWarehouseCenter : kWarehouseCenter, wy = w >= 2 ? -kWarehouseCenter : kWarehouseCenter;
            kind = RENDER_FAN; nv = 4;
            put(0, 1.0, 1.0, kWarehouseRadius, 1.0, 0.0, wx, wy); put(1, -1.0, 1.0, kWarehouseRadius, 1.0, 0.0, wx, wy);
            put(2, -1.0, -1.0, kWarehouseRadius, 1.0, 0.0, wx, wy); put(3, 1.0, -1.0, kWarehouseRadius, 1.0, 0.0, wx, wy);
            cr = w == 0 ? 52.0f / 255.0f : w == 1 ? 1.0f : w == 2 ? 149.0f / 255.0f : 134.0f / 255.0f;      // environment.py:44-49, as f32
            cg = w == 0 ? 127.0f / 255.0f : w == 1 ? 34.0f / 255.0f : w == 2 ? 117.0f / 255.0f : 110.0f / 255.0f;
            cb = w == 0 ? 212.0f / 255.0f : w == 1 ? 34.0f / 255.0f : w == 2 ? 205.0f / 255.0f : 68.0f / 255.0f;
            ca = busy ? 0.6f : 0.3f;
        } else if (tid < base_view) {                                        // obstacles (:1056-1061)
            const int o = tid - 5;
            const double *ob = st + 2 * Nc;
            kind = RENDER_NGON; nv = 72;
            q[0] = ob[o]; q[1] = ob[No + o]; q[2] = ob[2 * No + o];
            cr = cg = cb = 0.3f;
        } else if (tid < base_cam) {                                         // sector and field of view (:1128-1147)
            const int c = tid - base_view;
            const double *cm = cams + c * kRenderCamWords;
            kind = RENDER_VIEW; aux = c;
            x0 = cm[0] - cm[4]; x1 = cm[0] + cm[4]; y0 = cm[1] - cm[4]; y1 = cm[1] + cm[4];
            cr = (cam_flags[c] & 1u) ? 0.0f : 0.6f; cg = 0.6f; cb = 0.0f; ca = 0.25f;      // (the polygon's; the sector's is a constant)
        } else if (tid < base_marker) {                                      // camera images (:1063-1080, 1149-1156)
            const int c = (tid - base_cam) / 3, part = (tid - base_cam) - 3 * c;
            const double cx = st[c], cy = st[Nc + c], rad = p.cam_radius;
            if (part == 0) {
                kind = RENDER_NGON; nv = 72;
                q[0] = cx; q[1] = cy; q[2] = rad;
                sincos_deg(dy[c], q[6], q[5]);                               // (the base turns with the image: a 72-gon is no circle)
                const bool perceived = (cam_flags[c] >> 1) & 1u;             // entities.py:236-237
                cr = perceived ? 0.6f : 0.1f; cg = 0.2f; cb = perceived ? 0.1f : 0.6f;
            } else {
                double sn, cs;
                sincos_deg(dy[c], sn, cs);
                kind = RENDER_FAN; nv = 4;
                if (part == 1) {
                    put(0, 0.8, 0.6, rad, cs, sn, cx, cy); put(1, -0.8, 0.6, rad, cs, sn, cx, cy); put(2, -0.8, -0.6, rad, cs, sn, cx, cy); put(3, 0.8, -0.6, rad, cs, sn, cx, cy);
                    cr = cg = cb = 1.0f; ca = 0.75f;
                } else {
                    put(0, 0.7, 0.3, rad, cs, sn, cx, cy); put(1, 1.2, 0.3, rad, cs, sn, cx, cy); put(2, 1.2, -0.3, rad, cs, sn, cx, cy); put(3, 0.7, -0.3, rad, cs, sn, cx, cy);
                    cr = cg = cb = 0.1f; ca = 0.75f;
                }
            }
        } else if (tid < base_target) {                                      // tracked markers (:1108-1113, 1158-1161)
            const int t = tid - base_marker;
            if ((*tracked_bits >> t) & 1u) {
                kind = RENDER_NGON; nv = 15;
                q[0] = dy[2 * Nc + t]; q[1] = dy[2 * Nc + Nt + t]; q[2] = 1.2 * kTargetRenderRadius;
                cr = 1.0f; cg = 1.0f; cb = 0.0f;
            }
        } else {                                                             // targets and their no-bounty overlays (:1084-1106, 1163-1174)
            const int t = (tid - base_target) >> 1, overlay = (tid - base_target) & 1;
            const int goal = (di[t * TI_STRIDE + TI_GW] & 0xff) - 1;
            if (!overlay || (goal >= 0 && di[t * TI_STRIDE + TI_BOUNTY] == 0)) {
                const bool high = (reinterpret_cast<const uint64_t *>(st)[3 * Nc + 3 * No] >> t) & 1ull;      // capacity 2
                const double heading = a.headings ? a.headings[(int64_t)k * Nt + t] : 0.0;
                const double tx = dy[2 * Nc + t], tyy = dy[2 * Nc + Nt + t], scale = overlay ? 0.4 * kTargetRenderRadius : kTargetRenderRadius;
                double sn, cs;
                sincos_deg(heading, sn, cs);
                kind = RENDER_FAN;
                if (!high) {
                    nv = 6;
                    put(0, 1.0, 0.0, scale, cs, sn, tx, tyy); put(1, -0.2, 0.6, scale, cs, sn, tx, tyy); put(2, -0.8, 0.6, scale, cs, sn, tx, tyy);
                    put(3, -0.4, 0.0, scale, cs, sn, tx, tyy); put(4, -0.8, -0.6, scale, cs, sn, tx, tyy); put(5, -0.2, -0.6, scale, cs, sn, tx, tyy);
                } else {
                    nv = 5;
                    put(0, 1.0, 0.0, scale, cs, sn, tx, tyy); put(1, 0.3, 0.6, scale, cs, sn, tx, tyy); put(2, -0.8, 0.6, scale, cs, sn, tx, tyy);
                    put(3, -0.8, -0.6, scale, cs, sn, tx, tyy); put(4, 0.3, -0.6, scale, cs, sn, tx, tyy);
                }
                if (overlay) { cr = cg = cb = 1.0f; ca = 0.66f; }
                else if (goal < 0) { cr = 0.2f; cg = 0.6f; cb = 0.2f; }      // entities.py:549
                else {
                    cr = goal == 0 ? 52.0f / 255.0f : goal == 1 ? 1.0f : goal == 2 ? 149.0f / 255.0f : 134.0f / 255.0f;
                    cg = goal == 0 ? 127.0f / 255.0f : goal == 1 ? 34.0f / 255.0f : goal == 2 ? 117.0f / 255.0f : 110.0f / 255.0f;
                    cb = goal == 0 ? 212.0f / 255.0f : goal == 1 ? 34.0f / 255.0f : goal == 2 ? 205.0f / 255.0f : 68.0f / 255.0f;
                }
            }
        }
        if (kind == RENDER_NGON) {                                           // centre, radius, then the squares of the two deciding radii
            const double rad = q[2];
            const double inner = rad * (nv == 72 ? unit[2 * 1] : unit[2 * 72 + 2]);      // r cos(360 / n): inside the apothem r cos(180 / n)
            q[3] = rad * rad * (1.0 + 1e-12); q[4] = inner * inner;
            if (!(tid >= base_cam && tid < base_marker)) { q[5] = 1.0; q[6] = 0.0; }      // (cos, sin) of the polygon's turn: the camera bases' only
            x0 = q[0] - rad; x1 = q[0] + rad; y0 = q[1] - rad; y1 = q[1] + rad;
        }
        q[12] = x0; q[13] = x1; q[14] = y0; q[15] = y1;
        rgba[0] = cr; rgba[1] = cg; rgba[2] = cb; rgba[3] = ca;
        meta[0] = kind; meta[1] = nv; meta[2] = aux; meta[3] = 0;
    }
    __syncthreads();

    // ---------------------------------------------------------------------------------------------- 2: the slots whose box meets the tile's, in list order
    const double pitch = 2.0 * kRenderBound / (double)S;
    const int c0 = tx * kRenderTile, r0 = ty * kRenderTile;
    {
        const double tx0 = -kRenderBound + ((double)c0 + 0.5) * pitch, tx1 = -kRenderBound + ((double)(c0 + kRenderTile - 1) + 0.5) * pitch;
        const double ty1 = kRenderBound - ((double)r0 + 0.5) * pitch, ty0 = kRenderBound - ((double)(r0 + kRenderTile - 1) + 0.5) * pitch;
        bool hit = false;
        if (tid < slots) {
            const double *q = prims + tid * kRenderPrimWords;
            hit = reinterpret_cast<const int32_t *>(q + 20)[0] != RENDER_NONE && q[12] <= tx1 && q[13] >= tx0 && q[14] <= ty1 && q[15] >= ty0;
        }
        const unsigned long long ballot = __ballot(hit);
        if (lane == 0) wave_hits[wave] = (uint32_t)__popcll(ballot);
        __syncthreads();
        int before = 0;
        for (int w = 0; w < 4; ++w) before += w < wave ? (int)wave_hits[w] : 0;
        if (hit) list[before + __popcll(ballot & ((1ull << lane) - 1ull))] = (uint16_t)tid;
        __syncthreads();
    }
    const int listed = (int)(wave_hits[0] + wave_hits[1] + wave_hits[2] + wave_hits[3]);

    // ---------------------------------------------------------------------------------------------- 2b: the pairs of the trace whose arrow can touch the tile, in the wrapper's order
    double *arrows = reinterpret_cast<double *>(render_lds + render_lds_bytes(Nc, Nt, No));
    uint16_t *pairs = reinterpret_cast<uint16_t *>(arrows + kRenderArrowChunk * kRenderArrowWords);      // team << 8 | sender << 4 | recipient
    uint32_t *pair_hits = reinterpret_cast<uint32_t *>(pairs + kRenderMaxPairs);
    int kept = 0, split = -1;                                                // split: the list position the arrows go in front of (-1: there are none)
    if (a.duration > 0) {
        const int32_t episode = (di + Nt * TI_STRIDE)[EI_EPISODE];
        const int nnc = a.trace[0] && a.trace_tags[0][env] == episode ? Nc * Nc : 0;
        const int nnt = a.trace[1] && a.trace_tags[1][env] == episode ? Nt * Nt : 0;
        const double pad = kArrowHead + kArrowOffset + kArrowHalfWidth * pitch;
        const double tx0 = -kRenderBound + ((double)c0 + 0.5) * pitch - pad, tx1 = -kRenderBound + ((double)(c0 + kRenderTile - 1) + 0.5) * pitch + pad;
        const double ty1 = kRenderBound - ((double)r0 + 0.5) * pitch + pad, ty0 = kRenderBound - ((double)(r0 + kRenderTile - 1) + 0.5) * pitch - pad;
        for (int base = 0; base < nnc + nnt; base += 256) {                  // (the same trip count in every lane)
            const int j = base + tid;
            bool hit = false;
            int code = 0;
            if (j < nnc + nnt) {
                const int team = j >= nnc, jj = team ? j - nnc : j, n = team ? Nt : Nc, s = jj / n, r = jj - s * n;
                if (s != r && a.trace[team][env * (n * n) + jj] > 0) {
                    const double *xs = team ? dy + 2 * Nc : st, *ys = xs + n;
                    const double sx = xs[s], sy = ys[s], rx = xs[r], ry = ys[r];
                    hit = !(sx == rx && sy == ry) && (sx < rx ? sx : rx) <= tx1 && (sx > rx ? sx : rx) >= tx0 && (sy < ry ? sy : ry) <= ty1 && (sy > ry ? sy : ry) >= ty0;
                }
                code = team << 8 | s << 4 | r;
            }
            const unsigned long long ballot = __ballot(hit);
            if (lane == 0) pair_hits[wave] = (uint32_t)__popcll(ballot);
            __syncthreads();
            int before = kept;
            for (int w = 0; w < 4; ++w) before += w < wave ? (int)pair_hits[w] : 0;
            if (hit) pairs[before + __popcll(ballot & ((1ull << lane) - 1ull))] = (uint16_t)code;
            kept += (int)(pair_hits[0] + pair_hits[1] + pair_hits[2] + pair_hits[3]);
            __syncthreads();
        }
        if (kept > 0) for (split = 0; split < listed && (int)list[split] < 5 + No; ++split) {}
    }

    // ---------------------------------------------------------------------------------------------- 3: the pixel walks the list
    const int pc = c0 + (tid & (kRenderTile - 1)), pr = r0 + (tid >> 4);
    const double px = -kRenderBound + ((double)pc + 0.5) * pitch, py = kRenderBound - ((double)pr + 0.5) * pitch;
    float fr = 1.0f, fg = 1.0f, fb = 1.0f;
    for (int i = 0; i <= listed; ++i) {
        if (i == split) {                                                    // the arrows' list position: behind the static geoms (the same in every lane)
            const double half = kArrowHalfWidth * pitch;
            for (int first = 0; first < kept; first += kRenderArrowChunk) {
                const int chunk = kept - first < kRenderArrowChunk ? kept - first : kRenderArrowChunk;
                if (tid < chunk) {                                           // draw_arrow (render_communication.py:66-92) of one pair
                    const int code = pairs[first + tid], team = code >> 8, s = (code >> 4) & 15, r = code & 15, n = team ? Nt : Nc;
                    const double *xs = team ? dy + 2 * Nc : st, *ys = xs + n;
                    const uint8_t *rem = a.trace[team] + env * (n * n);
                    const int remaining = rem[s * n + r];
                    const bool both = rem[r * n + s] > 0;
                    const double sx = xs[s], sy = ys[s], ex = xs[r], ey = ys[r];
                    double vx = ex - sx, vy = ey - sy;
                    const double norm = sqrt(vx * vx + vy * vy);
                    const double shrink = (norm - kArrowHead) / norm, scale = 0.9 > shrink ? 0.9 : shrink;
                    vx = vx * scale; vy = vy * scale;
                    double v1x = 0.04 * vx + 0.015 * vy, v1y = -0.015 * vx + 0.04 * vy, v2x = 0.04 * vx + -0.015 * vy, v2y = 0.015 * vx + 0.04 * vy;
                    const double n1 = kArrowHead / sqrt(v1x * v1x + v1y * v1y), n2 = kArrowHead / sqrt(v2x * v2x + v2y * v2y);
                    const double k1 = 1.0 < n1 ? 1.0 : n1, k2 = 1.0 < n2 ? 1.0 : n2;
                    v1x = v1x * k1; v1y = v1y * k1; v2x = v2x * k2; v2y = v2y * k2;
                    double ax = ex - vx, ay = ey - vy, bx = sx + vx, by = sy + vy;      // start, end = end - vec, start + vec
                    if (both) {
                        double ux = 0.0 * vx + -1.0 * vy, uy = 1.0 * vx + 0.0 * vy;
                        const double ku = kArrowOffset / sqrt(ux * ux + uy * uy);
                        ux = ux * ku; uy = uy * ku;
                        ax = ax + ux; ay = ay + uy; bx = bx + ux; by = by + uy;
                    }
                    double *w = arrows + tid * kRenderArrowWords;
                    w[0] = ax; w[1] = ay; w[2] = bx; w[3] = by; w[4] = bx - v1x; w[5] = by - v1y; w[6] = bx - v2x; w[7] = by - v2y;
                    const double alpha = 1.2 * (double)remaining / (double)a.duration;
                    reinterpret_cast<float *>(w + 8)[0] = (float)(1.0 < alpha ? 1.0 : alpha);
                    reinterpret_cast<int32_t *>(w + 8)[1] = (both ? 2 : 3) | team << 2;
                }
                __syncthreads();
                for (int j = 0; j < chunk; ++j) {
                    const double *w = arrows + j * kRenderArrowWords;
                    const float al = reinterpret_cast<const float *>(w + 8)[0];
                    const int meta = __builtin_amdgcn_readfirstlane(reinterpret_cast<const int32_t *>(w + 8)[1]), lines = meta & 3;
                    const float red = (meta >> 2) ? 1.0f : 0.0f, blue = (meta >> 2) ? 0.0f : 1.0f;      // targets red, cameras blue
                    for (int l = 0; l < lines; ++l) {
                        const double *from = l == 0 ? w : w + 2 + 2 * l;
                        if (render_dash(px, py, from[0], from[1], w[2], w[3], half, pitch)) { fr = render_blend(fr, red, al); fg = render_blend(fg, 0.0f, al); fb = render_blend(fb, blue, al); }
                    }
                }
                __syncthreads();
            }
        }
        if (i == listed) break;
        const double *q = prims + (int)list[i] * kRenderPrimWords;
        const float *rgba = reinterpret_cast<const float *>(q + 18);
        const int32_t *meta = reinterpret_cast<const int32_t *>(q + 20);
        const int kind = __builtin_amdgcn_readfirstlane(meta[0]), nv = __builtin_amdgcn_readfirstlane(meta[1]);
        bool in = false;
        if (kind == RENDER_FAN) {
            for (int j = 1; j + 1 < nv; ++j) in = in || render_in_triangle(px, py, q[0], q[1], q[2 * j], q[2 * j + 1], q[2 * j + 2], q[2 * j + 3]);
        } else if (kind == RENDER_NGON) {
            const double wx = px - q[0], wy = py - q[1], d2 = wx * wx + wy * wy;
            if (d2 <= q[4]) in = true;
            else if (d2 <= q[3]) {                                           // the ring between the two circles: the edges, counter-clockwise, in the polygon's own frame
                const double dx = q[5] * wx + q[6] * wy, dyy = q[5] * wy - q[6] * wx;
                const double *u = unit + (nv == 72 ? 0 : 2 * 72);
                const double rad = q[2];
                bool all = true;
                for (int j = 0; j < nv; ++j) {
                    const int j1 = j + 1 == nv ? 0 : j + 1;
                    const double ax = u[2 * j] * rad, ay = u[2 * j + 1] * rad, bx = u[2 * j1] * rad, by = u[2 * j1 + 1] * rad;
                    all = all && render_cross(bx - ax, by - ay, dx - ax, dyy - ay) >= 0.0;
                }
                in = all;
            }
        } else if (kind == RENDER_LOOP) {                                    // within half a width of the nearest segment
            const double half = q[16];
            double best = INFINITY;
            for (int j = 0; j < nv; ++j) {
                const int j1 = j + 1 == nv ? 0 : j + 1;
                const double ax = q[2 * j], ay = q[2 * j + 1], ex = q[2 * j1] - ax, ey = q[2 * j1 + 1] - ay;
                const double t = clipd(((px - ax) * ex + (py - ay) * ey) / (ex * ex + ey * ey), 0.0, 1.0);
                const double ox = px - (ax + t * ex), oy = py - (ay + t * ey), d2 = ox * ox + oy * oy;
                best = d2 < best ? d2 : best;
            }
            in = best <= half * half;
        } else if (kind == RENDER_VIEW) {
            const int c = __builtin_amdgcn_readfirstlane(meta[2]);
            const double *cm = cams + c * kRenderCamWords;
            const double dx = px - cm[0], dyy = py - cm[1], sight = cm[4];
            const int64_t item = env * Nc + c;
            int n = a.knot_count[item];
            n = n > p.kmax ? p.kmax : n;
            bool in_sector = false;
            if (n >= 2 && dx * dx + dyy * dyy <= sight * sight * (1.0 + 1e-12) &&
                render_cross(cm[8], cm[9], dx, dyy) >= 0.0 && render_cross(dx, dyy, cm[10], cm[11]) >= 0.0) {      // inside the circle, between the flanks (theta <= 180)
                const double2 *kn = a.knots + item * p.kmax;
                const uint16_t *bk = a.bucket + item * p.nbucket;
                double ang = (dx == 0.0 && dyy == 0.0) ? 0.0 : atan2_deg(dyy, dx);
                if (!(ang < 180.0)) ang -= 360.0;
                if (!(ang >= -180.0)) ang = -180.0;
                int d = (int)floor(ang + 180.0);                             // lut_lookup's start: bucket[d] = the last knot at or below d - 180 degrees
                d = d < 1 ? 1 : (d > 359 ? 359 : d);
                int lo = bk[d - 1], hi = bk[d + 2 > 360 ? 360 : d + 2];
                hi = hi > n - 1 ? n - 1 : hi;
                lo = lo > hi ? hi : lo;
                while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (kn[mid].x <= ang) lo = mid; else hi = mid; }
                if (kn[hi].x <= ang) lo = hi;
                lo = lo > n - 2 ? n - 2 : lo;
                const double2 k0 = kn[lo], k1 = kn[lo + 1];                  // k0.x <= ang < k1.x: the wedge's knots, unless a sector end comes first
                const double theta = cm[3];
                double rel = ang - cm[2];
                rel = rel < 0.0 ? rel + 360.0 : rel;
                if (rel > theta) rel = rel - theta < 360.0 - rel ? theta : 0.0;      // (a bearing that rounded across a flank)
                const bool knot0 = ang - k0.x < rel, knot1 = k1.x - ang < theta - rel;
                double cs0 = cm[8], sn0 = cm[9], cs1 = cm[10], sn1 = cm[11];
                if (knot0) sincos_deg(k0.x, sn0, cs0);
                if (knot1) sincos_deg(k1.x, sn1, cs1);
                const double rho0 = knot0 ? clipd(k0.y, cm[5], sight) : cm[6], rho1 = knot1 ? clipd(k1.y, cm[5], sight) : cm[7];
                {   // the sector's far edge: both ends at sight_range
                    const double ax = sight * cs0, ay = sight * sn0, bx = sight * cs1, by = sight * sn1;
                    in_sector = render_cross(bx - ax, by - ay, dx - ax, dyy - ay) >= 0.0;
                }
                const double ax = rho0 * cs0, ay = rho0 * sn0, bx = rho1 * cs1, by = rho1 * sn1;
                in = render_cross(bx - ax, by - ay, dx - ax, dyy - ay) >= 0.0;
            }
            if (in_sector) { fr = render_blend(fr, 0.0f, 0.1f); fg = render_blend(fg, 0.6f, 0.1f); fb = render_blend(fb, 0.8f, 0.1f); }      // environment.py:1145
        }
        if (in) {
            const float al = rgba[3];
            fr = render_blend(fr, rgba[0], al); fg = render_blend(fg, rgba[1], al); fb = render_blend(fb, rgba[2], al);
        }
    }

    // ---------------------------------------------------------------------------------------------- 4: the frame
    const uint32_t qr = render_quantise(fr), qg = render_quantise(fg), qb = render_quantise(fb);
    uint8_t *frame = a.out + (int64_t)k * S * S * 3;
    if constexpr (kWide) {
        uint8_t *px3 = image + tid * 3;                                      // (row tid >> 4, 48 bytes a row)
        px3[0] = (uint8_t)qr; px3[1] = (uint8_t)qg; px3[2] = (uint8_t)qb;
        __syncthreads();
        if (tid < kRenderTile * 3) {
            const int row = tid / 3, piece = tid - 3 * row;
            const uint4 v = *reinterpret_cast<const uint4 *>(image + row * (kRenderTile * 3) + piece * 16);
            *reinterpret_cast<uint4 *>(frame + ((int64_t)(r0 + row) * S + c0) * 3 + piece * 16) = v;
        }
    } else if (pr < S && pc < S) {
        uint8_t *o = frame + ((int64_t)pr * S + pc) * 3;
        o[0] = (uint8_t)qr; o[1] = (uint8_t)qg; o[2] = (uint8_t)qb;
    }
}

// render_kernel on `blocks` tiles with `lds` bytes of dynamic LDS; returns the launch's error
hipError_t launch_render(bool wide, unsigned blocks, size_t lds, hipStream_t stream, const Params *params, const RenderArgs &a);

}  // namespace mate
