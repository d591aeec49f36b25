// Pictures of fields on the device: the 2 x 3 panels of plot_bubbleml and the strips of the wandb_*_plotter functions
// (bubbleformer/utils/plot_utils.py), fields in, uint8 RGB images out.  DESIGN.md section 19 has the layout and the rules; the numpy
// restatement tests/render_restatement.py pins every byte.
//
//   bf_render_ranges   {n, sum, sum of squares, min, max} in fp64 of the signed distance, the temperature and the speed of a set of frames:
//                      every workgroup sweeps a contiguous share, a second launch adds the workgroup rows in row order (no atomics).
//   bf_render_tiles    one launch for all images of a call.  A thread makes four horizontally adjacent pixels and stores them as three
//                      32-bit words (image widths are multiples of 4: no byte-wise tail).
//
// The colour index is matplotlib's: t = (x - vmin) / (vmax - vmin) in fp64, floor(256 t) clamped to 0 .. 255.  The difference and the
// quotient are single correctly rounded operations and the product with 256 is exact, so numpy gives the same index: this file is
// compiled without fused contraction, without fast-math and with the exact divide (Makefile).
#include "bf_common.h"

namespace {
constexpr int RN_NT = 256;
constexpr int RR_ROWS = 64;         // workgroups per quantity in bf_render_ranges
constexpr uint32_t RN_WHITE = 0xFFFFFFu;
constexpr double RN_INF = __builtin_huge_val();

// ---------------------------------------------------------------------------------------------------------------- ranges
__global__ void __launch_bounds__(RN_NT) render_ranges_kernel(const float* __restrict__ src, long frames, int C, long HW, int c_sdf, int c_temp,
                                                             int c_velx, int c_vely, double* __restrict__ part) {
    __shared__ double red[RN_NT / 64][4];      // several values at once in this kernel's own order, which its restatement's bits pin: not bf_common.h's block_reduce
    const int qn = blockIdx.y;                                                      // 0 signed distance, 1 temperature, 2 speed
    const int ca = qn == 0 ? c_sdf : qn == 1 ? c_temp : c_velx, cb = qn == 2 ? c_vely : 0;
    const long n = frames * HW;
    const long per = ((n + RR_ROWS - 1) / RR_ROWS + 3) & ~3L;                       // a multiple of 4: whole 16-byte groups when HW is one
    const long lo = (long)blockIdx.x * per, hi = min(n, lo + per);
    double s1 = 0.0, s2 = 0.0, mn = RN_INF, mx = -RN_INF;
    auto take = [&](double d) { s1 += d; s2 += d * d; mn = fmin(mn, d); mx = fmax(mx, d); };        // fmin / fmax drop a NaN, the sums keep it
    auto speed = [](float u, float v) { return __dsqrt_rn((double)u * (double)u + (double)v * (double)v); };
    if (ca >= 0 && cb >= 0) {
        if ((HW & 3) == 0 && (((uintptr_t)src) & 15) == 0) {                        // a group of 4 never crosses a frame
            for (long i = lo + 4L * threadIdx.x; i < hi; i += 4L * RN_NT) {
                const long f = i / HW, base = f * C * HW + (i - f * HW);
                const float4 a = *reinterpret_cast<const float4*>(src + base + ca * HW);
                if (qn == 2) {
                    const float4 b = *reinterpret_cast<const float4*>(src + base + cb * HW);
                    take(speed(a.x, b.x)); take(speed(a.y, b.y)); take(speed(a.z, b.z)); take(speed(a.w, b.w));
                } else { take(a.x); take(a.y); take(a.z); take(a.w); }
            }
        } else {
            for (long i = lo + threadIdx.x; i < hi; i += RN_NT) {
                const long f = i / HW, base = f * C * HW + (i - f * HW);
                take(qn == 2 ? speed(src[base + ca * HW], src[base + cb * HW]) : (double)src[base + ca * HW]);
            }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { s1 += __shfl_xor(s1, o, 64); s2 += __shfl_xor(s2, o, 64); mn = fmin(mn, __shfl_xor(mn, o, 64)); mx = fmax(mx, __shfl_xor(mx, o, 64)); }
    if ((threadIdx.x & 63) == 0) { double* r = red[threadIdx.x >> 6]; r[0] = s1; r[1] = s2; r[2] = mn; r[3] = mx; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double a = 0.0, b = 0.0, c = RN_INF, e = -RN_INF;
        for (int w = 0; w < RN_NT / 64; ++w) { a += red[w][0]; b += red[w][1]; c = fmin(c, red[w][2]); e = fmax(e, red[w][3]); }
        double* o = part + ((long)qn * RR_ROWS + blockIdx.x) * 4;
        o[0] = a; o[1] = b; o[2] = c; o[3] = e;
    }
}
__global__ void __launch_bounds__(64) render_ranges_finish_kernel(const double* __restrict__ part, double n, int c_sdf, int c_temp, int c_velx, int c_vely,
                                                                 double* __restrict__ out) {
    const int qn = threadIdx.x;
    if (qn >= 3) return;
    const bool present = qn == 0 ? c_sdf >= 0 : qn == 1 ? c_temp >= 0 : (c_velx >= 0 && c_vely >= 0);
    double a = 0.0, b = 0.0, c = RN_INF, e = -RN_INF;
    for (int r = 0; r < RR_ROWS; ++r) { const double* q = part + ((long)qn * RR_ROWS + r) * 4; a += q[0]; b += q[1]; c = fmin(c, q[2]); e = fmax(e, q[3]); }
    double* o = out + qn * 5;
    o[0] = present ? n : 0.0; o[1] = a; o[2] = b; o[3] = c; o[4] = e;
}

// ---------------------------------------------------------------------------------------------------------------- tiles
struct RenderArgs { bf_render_tile t[BF_RENDER_MAX_TILES]; int n; };

// matplotlib's Normalize + Colormap.__call__: the packed colour of x, white for a NaN
__device__ __forceinline__ uint32_t colour_of(double x, double vmin, double vmax, const uint32_t* lut) {
    if (vmax == vmin) return lut[0];
    const double t = (x - vmin) / (vmax - vmin);
    if (t != t) return RN_WHITE;
    const double k = t * 256.0;
    return lut[k >= 256.0 ? 255 : k < 0.0 ? 0 : (int)floor(k)];
}

__device__ __forceinline__ bool liquid(const float* f, int W, int i, int j) { return f[(long)i * W + j] < 0.f; }
// a liquid cell with an in-range 4-neighbour that is not liquid
__device__ __forceinline__ bool edge_cell(const float* f, int H, int W, int i, int j) {
    if (!liquid(f, W, i, j)) return false;
    return (i > 0 && !liquid(f, W, i - 1, j)) || (i + 1 < H && !liquid(f, W, i + 1, j)) || (j > 0 && !liquid(f, W, i, j - 1)) ||
           (j + 1 < W && !liquid(f, W, i, j + 1));
}
// the 3 x 3 dilation of the edge cells
__device__ __forceinline__ bool outlined(const float* f, int H, int W, int i, int j) {
    for (int ii = max(i - 1, 0); ii <= min(i + 1, H - 1); ++ii)
        for (int jj = max(j - 1, 0); jj <= min(j + 1, W - 1); ++jj)
            if (edge_cell(f, H, W, ii, jj)) return true;
    return false;
}

// squared distance of (px, py) to the stroke from (ax, ay) to (bx, by)
__device__ __forceinline__ double stroke_d2(double px, double py, double ax, double ay, double bx, double by) {
    const double ex = bx - ax, ey = by - ay, wx = px - ax, wy = py - ay;
    const double l2 = ex * ex + ey * ey;
    double t = l2 > 0.0 ? (wx * ex + wy * ey) / l2 : 0.0;
    t = fmin(fmax(t, 0.0), 1.0);
    const double dx = wx - t * ex, dy = wy - t * ey;
    return dx * dx + dy * dy;
}

// is the pixel centre (px, py) of a speed tile on the arrow of its own block of cells or of one of the 8 blocks around it
__device__ bool on_arrow(const float* u, const float* v, const float* mask, const bf_render_geom& g, double vmax, int i, int j, double px, double py) {
    if (!(vmax > 0.0)) return false;
    const int st = g.stride, bi = i / st, bj = j / st;
    const double s = (double)g.scale, full = 0.9 * st * s, hw = g.stroke;
    const double reach = 0.5 * full + hw + 1e-3;                                // every stroke lies within half the longest arrow of its anchor
    for (int bb = bi - 1; bb <= bi + 1; ++bb) {
        const int ai = bb * st + st / 2;
        if (bb < 0 || ai >= g.H) continue;
        for (int ba = bj - 1; ba <= bj + 1; ++ba) {
            const int aj = ba * st + st / 2;
            if (ba < 0 || aj >= g.W) continue;
            const double cx = (aj + 0.5) * s, cy = (g.H - 1 - ai + 0.5) * s;
            if ((px - cx) * (px - cx) + (py - cy) * (py - cy) > reach * reach) continue;
            const long at = (long)ai * g.W + aj;
            double uu = (double)u[at], vv = (double)v[at];
            if (mask && mask[at] > 0.f) uu = vv = 0.0;
            const double q = __dsqrt_rn(uu * uu + vv * vv);
            if (!(q > 0.0) || !(q < RN_INF)) continue;
            const double len = full * fmin(q / vmax, 1.0), dx = uu / q, dy = -vv / q, h = 0.5 * len, k = 0.35 * len;
            const double tx = cx + h * dx, ty = cy + h * dy;
            // the head strokes leave the tip at +-150 degrees to d: cos = -sqrt(3)/2, sin = +-1/2
            const double c150 = -0.86602540378443864676, s150 = 0.5;
            const double lim = hw * hw;
            if (stroke_d2(px, py, cx - h * dx, cy - h * dy, tx, ty) <= lim) return true;
            if (stroke_d2(px, py, tx, ty, tx + k * (c150 * dx - s150 * dy), ty + k * (s150 * dx + c150 * dy)) <= lim) return true;
            if (stroke_d2(px, py, tx, ty, tx + k * (c150 * dx + s150 * dy), ty + k * (-s150 * dx + c150 * dy)) <= lim) return true;
        }
    }
    return false;
}

__global__ void __launch_bounds__(RN_NT) render_tiles_kernel(RenderArgs A, bf_render_geom g, long images, const uint8_t* __restrict__ lut_blues,
                                                            const uint8_t* __restrict__ lut_turbo, uint32_t* __restrict__ out) {
    __shared__ uint32_t lut[2][256];
    __shared__ bf_render_tile tiles[BF_RENDER_MAX_TILES];
    for (int k = threadIdx.x; k < 512; k += RN_NT) {
        const uint8_t* p = (k < 256 ? lut_blues : lut_turbo) + 3 * (k & 255);
        lut[k >> 8][k & 255] = (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16);
    }
    if (threadIdx.x < A.n) tiles[threadIdx.x] = A.t[threadIdx.x];
    __syncthreads();
    const int wq = g.img_w / 4, hs = g.H * g.scale, ws = g.W * g.scale;
    const long total = images * g.img_h * wq;
    for (long e = (long)blockIdx.x * RN_NT + threadIdx.x; e < total; e += (long)gridDim.x * RN_NT) {
        const long r = e / wq;
        const int q = (int)(e - r * wq), py = (int)(r % g.img_h);
        const long img = r / g.img_h;
        const int cy = py - g.oy, row = cy >= 0 ? cy / g.pitch_y : 0, ly = cy >= 0 ? cy % g.pitch_y : 0;
        const bool in_row = cy >= 0 && row < g.rows && ly < hs;
        const int i = g.H - 1 - ly / g.scale;                                       // row 0 of the field is the bottom row of the tile
        uint32_t c[4];
        long seen = -1;
        bool seen_outline = false;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            c[k] = RN_WHITE;
            const int cx = 4 * q + k - g.ox;
            if (!in_row || cx < 0) continue;
            const int col = cx / g.pitch_x, lx = cx % g.pitch_x;
            if (col >= g.cols) continue;
            const int slot = row * g.cols + col;
            const bf_render_tile& T = tiles[slot % A.n];
            const uint32_t* L = lut[T.kind == BF_RENDER_SDF ? 0 : 1];
            if (lx >= g.bar_dx && lx < g.bar_dx + g.bar_w) { c[k] = L[((hs - 1 - ly) * 256) / hs]; continue; }       // vmax on top
            if (lx >= ws) continue;
            const int j = lx / g.scale;
            const long off = img * T.frame_stride + (long)(slot / A.n) * T.slot_stride, at = (long)i * g.W + j;
            const double vmin = T.range[0], vmax = T.range[1];
            if (T.kind == BF_RENDER_SPEED) {
                const float* u = T.a + off;
                const float* v = T.b + off;
                const float* m = T.mask ? T.mask + img * T.mask_frame_stride + (long)(slot / A.n) * T.mask_slot_stride : nullptr;
                if (on_arrow(u, v, m, g, vmax, i, j, lx + 0.5, ly + 0.5)) continue;
                const double a = (double)u[at], b = (double)v[at];
                c[k] = colour_of(__dsqrt_rn(a * a + b * b), vmin, vmax, L);
            } else {
                const float* f = T.a + off;
                if (T.kind == BF_RENDER_SDF) {
                    const long key = (long)slot * hs * ws + at;                    // the same cell of the same tile as the pixel before
                    if (key != seen) { seen = key; seen_outline = outlined(f, g.H, g.W, i, j); }
                    if (seen_outline) { c[k] = 0u; continue; }
                }
                c[k] = colour_of((double)f[at], vmin, vmax, L);
            }
        }
        uint32_t* o = out + ((img * g.img_h + py) * (long)g.img_w * 3) / 4 + 3L * q;
        o[0] = c[0] | (c[1] << 24);
        o[1] = (c[1] >> 8) | (c[2] << 16);
        o[2] = (c[2] >> 16) | (c[3] << 8);
    }
}
}  // namespace

extern "C" int64_t bf_render_ranges_ws_doubles(void) { return 3L * RR_ROWS * 4; }
extern "C" int bf_render_ranges(const float* src, int64_t frames, int C, int H, int W, int c_sdf, int c_temp, int c_velx, int c_vely, double* out, double* ws,
                                bf_stream_t stream) {
    BF_REQUIRE(src && out && ws, "bf_render_ranges: null pointer");
    BF_REQUIRE(frames > 0 && C > 0 && H > 0 && W > 0, "bf_render_ranges: bad sizes");
    BF_REQUIRE(c_sdf >= -1 && c_sdf < C && c_temp >= -1 && c_temp < C && c_velx >= -1 && c_velx < C && c_vely >= -1 && c_vely < C,
               "bf_render_ranges: a channel index must be -1 (skip) or inside the frame");
    hipLaunchKernelGGL(render_ranges_kernel, dim3(RR_ROWS, 3), dim3(RN_NT), 0, (hipStream_t)stream, src, (long)frames, C, (long)H * W, c_sdf, c_temp, c_velx,
                       c_vely, ws);
    BF_CHECK_LAUNCH();
    hipLaunchKernelGGL(render_ranges_finish_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (const double*)ws, (double)frames * H * W, c_sdf, c_temp, c_velx,
                       c_vely, out);
    BF_CHECK_LAUNCH();
    return 0;
}

extern "C" int bf_render_tiles(const bf_render_tile* tiles, int ntiles, const bf_render_geom* geom, int64_t images, const uint8_t* lut_blues,
                               const uint8_t* lut_turbo, uint8_t* out, bf_stream_t stream) {
    BF_REQUIRE(tiles && geom && lut_blues && lut_turbo && out, "bf_render_tiles: null pointer");
    const bf_render_geom g = *geom;
    BF_REQUIRE(ntiles >= 1 && ntiles <= BF_RENDER_MAX_TILES && images > 0, "bf_render_tiles: 1 .. BF_RENDER_MAX_TILES tile descriptions, at least one image");
    BF_REQUIRE(g.H > 0 && g.W > 0 && g.scale > 0 && g.rows > 0 && g.cols > 0 && g.stride > 0 && g.stroke > 0.0, "bf_render_tiles: bad sizes");
    BF_REQUIRE((long)g.H * g.scale <= 32768 && (long)g.W * g.scale <= 32768 && (long)g.img_w * g.img_h * 3 < (1L << 31), "bf_render_tiles: image too large");
    BF_REQUIRE((g.rows * g.cols) % ntiles == 0, "bf_render_tiles: the slots of an image must be a whole number of rounds through the descriptions");
    BF_REQUIRE(g.ox >= 0 && g.oy >= 0 && g.bar_w >= 0 && g.bar_dx >= g.W * g.scale && g.pitch_x >= g.bar_dx + g.bar_w && g.pitch_y >= g.H * g.scale,
               "bf_render_tiles: a tile, its bar and its neighbour overlap");
    BF_REQUIRE(g.img_w > 0 && g.img_w % 4 == 0 && g.ox + (long)(g.cols - 1) * g.pitch_x + g.bar_dx + g.bar_w <= g.img_w &&
               g.oy + (long)(g.rows - 1) * g.pitch_y + (long)g.H * g.scale <= g.img_h, "bf_render_tiles: the image width must be a multiple of 4 and hold every tile");
    BF_REQUIRE(((uintptr_t)out & 3) == 0, "bf_render_tiles: the image must be 4-byte aligned");
    RenderArgs A;
    A.n = ntiles;
    for (int k = 0; k < BF_RENDER_MAX_TILES; ++k) A.t[k] = tiles[k < ntiles ? k : 0];
    for (int k = 0; k < ntiles; ++k) {
        BF_REQUIRE(tiles[k].a && tiles[k].range && tiles[k].kind >= BF_RENDER_SDF && tiles[k].kind <= BF_RENDER_SPEED, "bf_render_tiles: a tile needs its field, its range and a kind");
        BF_REQUIRE(tiles[k].kind != BF_RENDER_SPEED || tiles[k].b, "bf_render_tiles: a speed tile needs both velocity components");
    }
    const long total = (long)images * g.img_h * (g.img_w / 4);
    const long blocks = (total + RN_NT - 1) / RN_NT;
    hipLaunchKernelGGL(render_tiles_kernel, dim3((unsigned)(blocks < 262144 ? blocks : 262144)), dim3(RN_NT), 0, (hipStream_t)stream, A, g, (long)images, lut_blues,
                       lut_turbo, reinterpret_cast<uint32_t*>(out));
    BF_CHECK_LAUNCH();
    return 0;
}
