// The 16-bit form of the device clip store: [fields][total_frames][H][W] codes of 16 bits with one affine scale per
// SEGMENT -- all frames of one field of one file, nfields x nfiles of them, segment (field, file) at table index field * nfiles + file.
//
// The format, per segment (the only definition; tests/clip_q16_restatement.py restates it in np.float32):
//   lo, hi = the exact fp32 minimum and maximum of the segment's values
//   step   = fp32(((double)hi - (double)lo) / 65535.0),  inv = fp32(65535.0 / ((double)hi - (double)lo));  hi == lo: step = inv = 0
//   encode   q = (x - lo) * inv in fp32, one rounded difference and one rounded product, never fused;
//            code = clamp(rintf(q), 0, 65535), round half to even
//   decode   x^ = fp32(fp32((float)code * step) + lo): one rounded product, then one rounded sum, never an fma
// A constant segment decodes exactly, and so does lo (code 0).  |x^ - x| <= 0.53 step + 2^-24 max(|lo|, |hi|): half a step, six fp32
// roundings of at most 0.004 step each, and the final sum's rounding.  A value closer to zero than step / 2 may come back with the other
// sign (a dfun that close to the interface); nothing here works round that.
//
// Everything behind the decode -- the index map, the mirror's sign on the STORED value, clip_norm, the window, the Philox block of a
// sample -- is clip_store.h's and philox.h's, as the fp32 gathers of clip_store.hip use them: the gather of a q16 store has the bits of
// the fp32 gather of its decoded frames.
#include "clip_store.h"
#include "philox.h"
#include <algorithm>

namespace {
constexpr int NT = 256;

__device__ __forceinline__ float q16_decode(uint32_t code, float step, float lo) {
#pragma clang fp contract(off)
    const float prod = (float)code * step;
    return prod + lo;
}
__device__ __forceinline__ uint32_t q16_encode(float x, float lo, float inv) {
#pragma clang fp contract(off)
    const float diff = x - lo;
    const float q = diff * inv;
    return (uint32_t)fminf(fmaxf(rintf(q), 0.f), 65535.f);
}
// the file a frame of the store's frame axis belongs to, held inside the tables whatever the table says
__device__ __forceinline__ int q16_file(const int* __restrict__ frame_seg, long frame, int nfiles) { return min(max(frame_seg[frame], 0), nfiles - 1); }
}  // namespace

// ---------------------------------------------------------------------------- encode one staged chunk of one segment
// dst[i] = code(src[i]), i < n.  A thread takes four values: one 16-byte load and one 8-byte store when both pointers allow it, scalar
// accesses otherwise; the n % 4 values at the end are always scalar.
__global__ void __launch_bounds__(NT) clip_encode_q16_kernel(const float* __restrict__ src, uint16_t* __restrict__ dst, long n, float lo, float inv, int wide) {
    const long nq = n >> 2;
    for (long i = (long)blockIdx.x * NT + threadIdx.x; i < nq; i += (long)gridDim.x * NT) {
        if (wide) {
            const float4 v = *reinterpret_cast<const float4*>(src + 4 * i);
            const uint32_t c0 = q16_encode(v.x, lo, inv), c1 = q16_encode(v.y, lo, inv), c2 = q16_encode(v.z, lo, inv), c3 = q16_encode(v.w, lo, inv);
            *reinterpret_cast<uint2*>(dst + 4 * i) = make_uint2(c0 | (c1 << 16), c2 | (c3 << 16));
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) dst[4 * i + k] = (uint16_t)q16_encode(src[4 * i + k], lo, inv);
        }
    }
    if (blockIdx.x == 0 && threadIdx.x < (n & 3)) dst[4 * nq + threadIdx.x] = (uint16_t)q16_encode(src[4 * nq + threadIdx.x], lo, inv);
}
extern "C" int bf_clip_encode_q16(const float* src, uint16_t* dst, int64_t n, float lo, float inv, bf_stream_t stream) {
    BF_REQUIRE(src && dst, "bf_clip_encode_q16: null pointer");
    BF_REQUIRE(n > 0, "bf_clip_encode_q16: n must be positive");
    BF_REQUIRE(((uintptr_t)src % 4 == 0) && ((uintptr_t)dst % 2 == 0), "bf_clip_encode_q16: src must be 4-byte and dst 2-byte aligned");
    BF_REQUIRE(lo == lo && inv >= 0.f && inv <= 3.4028234664e38f, "bf_clip_encode_q16: lo must be a number and inv finite and >= 0");
    const int wide = ((uintptr_t)src % 16 == 0) && ((uintptr_t)dst % 8 == 0);
    const long nq = (long)(n >> 2);
    const int grid = (int)std::max<long>(1, std::min<long>((nq + NT - 1) / NT, 256L * 16));
    hipLaunchKernelGGL(clip_encode_q16_kernel, dim3(grid), dim3(NT), 0, (hipStream_t)stream, src, dst, (long)n, lo, inv, wide);
    BF_CHECK_LAUNCH();
    return 0;
}

// ---------------------------------------------------------------------------- decode a whole store
// dst [nfields][nframes][H][W] fp32 (contiguous) = the decoded codes.  Frames lie on the grid's y axis (field-major); the segment is looked up
// once per thread and frame.  Four codes are one 8-byte load and the four values one 16-byte store when H * W and the field stride are
// multiples of 4 and the pointers allow it.
__global__ void __launch_bounds__(NT) clip_decode_q16_kernel(const uint16_t* __restrict__ codes, long field_stride, const int* __restrict__ frame_seg,
                                                            const float* __restrict__ seg_lo, const float* __restrict__ seg_step, float* __restrict__ dst,
                                                            long nframes, int nfields, int nfiles, int px, int wide) {
    const long planes = (long)nfields * nframes;
    const int nq = (px + 3) >> 2;
    for (long p = blockIdx.y; p < planes; p += gridDim.y) {
        const int f = (int)(p / nframes);
        const long fr = p - (long)f * nframes;
        const int seg = f * nfiles + q16_file(frame_seg, fr, nfiles);
        const float lo = seg_lo[seg], st = seg_step[seg];
        const uint16_t* s = codes + (long)f * field_stride + fr * px;
        float* d = dst + p * px;
        for (int i = blockIdx.x * NT + threadIdx.x; i < nq; i += gridDim.x * NT) {
            if (wide) {                                                 // px is whole quads
                const uint2 v = *reinterpret_cast<const uint2*>(s + 4 * i);
                *reinterpret_cast<float4*>(d + 4 * i) = make_float4(q16_decode(v.x & 0xFFFFu, st, lo), q16_decode(v.x >> 16, st, lo),
                                                                    q16_decode(v.y & 0xFFFFu, st, lo), q16_decode(v.y >> 16, st, lo));
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (4 * i + k < px) d[4 * i + k] = q16_decode(s[4 * i + k], st, lo);
            }
        }
    }
}
extern "C" int bf_clip_decode_q16(const uint16_t* codes, int64_t field_stride, const int32_t* frame_seg, const float* seg_lo, const float* seg_step,
                                  float* dst, int64_t nframes, int nfields, int nfiles, int H, int W, bf_stream_t stream) {
    BF_REQUIRE(codes && frame_seg && seg_lo && seg_step && dst, "bf_clip_decode_q16: null pointer");
    BF_REQUIRE(nframes > 0 && nfields > 0 && nfiles > 0 && H > 0 && W > 0 && (int64_t)H * W < (1LL << 31) - 4 && field_stride >= nframes * (int64_t)H * W,
               "bf_clip_decode_q16: bad sizes");
    BF_REQUIRE(((uintptr_t)codes % 2 == 0) && ((uintptr_t)dst % 4 == 0), "bf_clip_decode_q16: the codes must be 2-byte and dst 4-byte aligned");
    const int px = H * W;
    const int wide = (px & 3) == 0 && (field_stride & 3) == 0 && ((uintptr_t)codes % 8 == 0) && ((uintptr_t)dst % 16 == 0);
    const long planes = (long)nfields * nframes;
    const int gx = std::max(1, std::min(((px + 3) / 4 + NT - 1) / NT, 64));
    const int gy = (int)std::min<long>(planes, 65535);
    hipLaunchKernelGGL(clip_decode_q16_kernel, dim3(gx, gy), dim3(NT), 0, (hipStream_t)stream, codes, (long)field_stride, (const int*)frame_seg, seg_lo, seg_step,
                       dst, (long)nframes, nfields, nfiles, px, wide);
    BF_CHECK_LAUNCH();
    return 0;
}

// ---------------------------------------------------------------------------- the gather, decoding as it reads
// What clip_gather_batch_kernel, clip_gather_unroll_kernel and clip_gather_augment_kernel (clip_store.hip) give on the decoded frames, from
// the codes, in one launch: the augment kernel's body -- samples on the grid's y axis, the sample's Philox block in front of its pixel loop,
// the unroll kernel's output layout and frame clamp -- with the decode in front of the mirror's sign.  Without an augment record the
// window is the whole output grid at the origin and nothing is mirrored, which is the plain and the unrolled gather's index map.
// The scale of a value is that of the frame actually READ (frame_seg[frame]), not of the sample's file: the frame clamp hands a sample
// whose later clips lie behind its file the next file's frames.  A thread's pixel loop walks (clip frame, channel) planes; the plane's
// frame, segment scale, constants, sign and row bases are looked up when the plane changes, never per pixel.
// A thread serves 4 output pixels of a row: one 8-byte load of four codes and one 16-byte store at the identity map when W, Wc and x0 are
// multiples of 4 (a mirrored quad is one aligned quad read back to front), scalar 2-byte loads otherwise, as the fp32 kernel's paths.
__global__ void __launch_bounds__(NT) clip_gather_q16_kernel(const uint16_t* __restrict__ codes, long field_stride, const int* __restrict__ frame_seg,
                                                            const float* __restrict__ seg_lo, const float* __restrict__ seg_step, int nfiles,
                                                            const long* __restrict__ idx, long nsamples, const long* __restrict__ first_tab, ClipSeg a, ClipSeg b,
                                                            const float* __restrict__ fluid_tab, const long* __restrict__ file_tab, int P,
                                                            float* __restrict__ fluid_out, int B, int H, int W, int Ho, int Wo, int unroll, long nframes,
                                                            ClipAugment g) {
    const int Hc = g.Hc, Wc = g.Wc;
    const int wq = (Wc + 3) / 4;
    const int plane = Hc * wq;                                          // quads of one (clip frame, channel) plane
    const long planes_a = (long)a.T * a.C, per = (planes_a + (long)b.T * b.C) * plane;
    const float sy = (float)H / (float)Ho, sx = (float)W / (float)Wo;
    const bool ident = Ho == H && Wo == W;
    const int Tc = b.T / unroll;
    if (fluid_out && blockIdx.x == 0 && blockIdx.y == 0)
        for (int i = threadIdx.x; i < B * P; i += NT) fluid_out[i] = fluid_tab[file_tab[min(max(idx[i / P], 0L), nsamples - 1)] * P + i % P];
    for (int bb = blockIdx.y; bb < B; bb += gridDim.y) {
        const long smp = min(max(idx[bb], 0L), nsamples - 1);
        bool flip = false;
        int x0 = (Wo - Wc) / 2, y0 = 0;
        if (!g.eval_view) {
            const Quad q = philox4x32_10(0xFFFFFFFFu, (uint32_t)(unsigned long)smp, g.draw, 0u, g.k0, g.k1);
            flip = (unsigned long long)q.w[0] < g.thr;
            x0 = (int)(((unsigned long long)q.w[1] * (unsigned long long)(Wo - Wc + 1)) >> 32);
            y0 = g.random_y ? (int)(((unsigned long long)q.w[2] * (unsigned long long)(Ho - Hc + 1)) >> 32) : 0;
        }
        const long first = first_tab[smp];
        const bool vec = ident && ((W | Wc | x0) & 3) == 0;            // the entry point has checked the codes' alignment and the field stride for this path
        long cur = -1;                                                  // the plane the values below belong to
        const uint16_t* src = nullptr;
        float* out = nullptr;
        float lo = 0.f, st = 0.f, d = 0.f, q = 1.f;
        bool neg = false;
        for (long r0 = (long)blockIdx.x * NT + threadIdx.x; r0 < per; r0 += (long)gridDim.x * NT) {
            const long pl = r0 / plane;
            const int rem = (int)(r0 - pl * plane);
            if (pl != cur) {
                cur = pl;
                const bool second = pl >= planes_a;
                const ClipSeg& sg = second ? b : a;
                const int tc = (int)(second ? pl - planes_a : pl);
                const int t = tc / sg.C, c = tc - t * sg.C;
                const long frame = min(first + sg.t0 + t, nframes - 1);
                const int j = second ? t / Tc : 0;
                const long orow = second ? ((long)j * B + bb) * Tc + (t - j * Tc) : (long)bb * sg.T + t;      // as the unroll kernel lays its rows out
                const int f = sg.field[c];
                const int seg = f * nfiles + q16_file(frame_seg, frame, nfiles);
                lo = seg_lo[seg]; st = seg_step[seg];
                d = sg.diff[c]; q = sg.dv[c];
                neg = flip && (second ? g.odd_b : g.odd_a)[c] != 0;
                src = codes + (long)f * field_stride + frame * H * (long)W;
                out = sg.out + (orow * sg.C + c) * Hc * (long)Wc;
            }
            const int y = rem / wq, xq = rem - y * wq;
            const uint16_t* row = src + (long)nearest_src(y0 + y, sy, H, ident) * W;
            float* dst = out + (long)y * Wc + 4 * xq;
            if (vec) {                                                  // 4 xq + 3 < Wc: the window is whole quads
                const uint2 v = *reinterpret_cast<const uint2*>(row + (flip ? x0 + Wc - 4 - 4 * xq : x0 + 4 * xq));
                const float v0 = q16_decode(v.x & 0xFFFFu, st, lo), v1 = q16_decode(v.x >> 16, st, lo);
                const float v2 = q16_decode(v.y & 0xFFFFu, st, lo), v3 = q16_decode(v.y >> 16, st, lo);
                const float e0 = flip ? v3 : v0, e1 = flip ? v2 : v1, e2 = flip ? v1 : v2, e3 = flip ? v0 : v3;
                *reinterpret_cast<float4*>(dst) = make_float4(clip_norm(neg ? -e0 : e0, d, q), clip_norm(neg ? -e1 : e1, d, q),
                                                              clip_norm(neg ? -e2 : e2, d, q), clip_norm(neg ? -e3 : e3, d, q));
            } else if ((Wc & 3) == 0) {                                 // whole quads at an origin or through a map that is not aligned: scalar loads, one 16-byte store
                float o[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int x = 4 * xq + k;
                    const float v = q16_decode(row[nearest_src(flip ? x0 + Wc - 1 - x : x0 + x, sx, W, ident)], st, lo);
                    o[k] = clip_norm(neg ? -v : v, d, q);
                }
                *reinterpret_cast<float4*>(dst) = make_float4(o[0], o[1], o[2], o[3]);
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int x = 4 * xq + k;
                    if (x < Wc) {
                        const float v = q16_decode(row[nearest_src(flip ? x0 + Wc - 1 - x : x0 + x, sx, W, ident)], st, lo);
                        dst[k] = clip_norm(neg ? -v : v, d, q);
                    }
                }
            }
        }
    }
}

extern "C" int bf_clip_gather_q16(const bf_clip_gather_q16_job* j, const bf_clip_augment* g, bf_stream_t stream) {
    BF_REQUIRE(j && j->codes && j->frame_seg && j->seg_lo && j->seg_step && j->idx && j->first_tab && j->in_field && j->in_diff && j->in_div && j->in_out &&
               j->out_field && j->out_diff && j->out_div && j->out_out && (!g || (g->in_odd && g->out_odd)), "bf_clip_gather_q16: null pointer");
    BF_REQUIRE(j->nsamples > 0 && j->nfiles > 0 && j->B > 0 && j->Tin > 0 && j->Tout > 0 && j->Cin > 0 && j->Cout > 0 && j->H > 0 && j->W > 0 && j->Ho > 0 &&
               j->Wo > 0 && j->Ho <= j->H && j->Wo <= j->W, "bf_clip_gather_q16: bad sizes");
    BF_REQUIRE(j->unroll >= 1 && j->unroll <= 1024 && j->nframes > 0 && j->field_stride >= j->nframes * (int64_t)j->H * j->W,
               "bf_clip_gather_q16: bad unroll count or frame count");
    BF_REQUIRE(!j->fluid_out || (j->fluid_tab && j->file_tab && j->P > 0), "bf_clip_gather_q16: the fluid rows need their table, the file table and P > 0");
    BF_REQUIRE(((uintptr_t)j->in_out % 16 == 0) && ((uintptr_t)j->out_out % 16 == 0), "bf_clip_gather_q16: the output buffers must be 16-byte aligned");
    if (g) {
        BF_REQUIRE(g->Hc >= 1 && g->Hc <= j->Ho && g->Wc >= 1 && g->Wc <= j->Wo, "bf_clip_gather_q16: the window must be 1 .. Ho by 1 .. Wo");
        BF_REQUIRE(g->flip_thr >= 0 && g->flip_thr <= (1LL << 32) && (g->crop_y == 0 || g->crop_y == 1) && (g->eval_view == 0 || g->eval_view == 1),
                   "bf_clip_gather_q16: bad flip threshold, crop_y or eval_view");
    }
    const int Hc = g ? g->Hc : j->Ho, Wc = g ? g->Wc : j->Wo;
    // rows are read four codes at a time when the map is the identity and W, Wc (and a sample's x0) are multiples of 4: every row then starts on 8 bytes
    const bool may_be_wide = j->Ho == j->H && j->Wo == j->W && ((j->W | Wc) & 3) == 0;
    BF_REQUIRE(((uintptr_t)j->codes % 2 == 0) && (!may_be_wide || ((uintptr_t)j->codes % 8 == 0 && (j->field_stride & 3) == 0)),
               "bf_clip_gather_q16: the codes must be 2-byte aligned, and 8-byte aligned with a field stride of whole quads where rows are read four codes at a time");
    BF_REQUIRE((int64_t)Hc * ((Wc + 3) / 4) < (1LL << 31), "bf_clip_gather_q16: the window must hold fewer than 2^31 quads");
    const ClipSeg a{(const int*)j->in_field, j->in_diff, j->in_div, j->in_out, j->Tin, j->Cin, 0};
    const ClipSeg b{(const int*)j->out_field, j->out_diff, j->out_div, j->out_out, j->unroll * j->Tout, j->Cout, j->Tin};
    const ClipAugment aug = g ? ClipAugment{(const int*)g->in_odd, (const int*)g->out_odd, (uint32_t)(uint64_t)g->seed, (uint32_t)((uint64_t)g->seed >> 32),
                                              (uint32_t)g->draw, (unsigned long long)g->flip_thr, Hc, Wc, g->crop_y, g->eval_view}
                               : ClipAugment{nullptr, nullptr, 0u, 0u, 0u, 0ULL, Hc, Wc, 0, 1};      // the whole grid at the origin, nothing drawn
    const long per = ((long)j->Tin * j->Cin + (long)j->unroll * j->Tout * j->Cout) * Hc * ((Wc + 3) / 4);
    const int gy = std::min(j->B, 65535);
    const int gx = (int)std::max<long>(1, std::min<long>((per + NT - 1) / NT, std::max(1, 256 * 16 / gy)));
    hipLaunchKernelGGL(clip_gather_q16_kernel, dim3(gx, gy), dim3(NT), 0, (hipStream_t)stream, j->codes, (long)j->field_stride, (const int*)j->frame_seg,
                       j->seg_lo, j->seg_step, j->nfiles, (const long*)j->idx, (long)j->nsamples, (const long*)j->first_tab, a, b, j->fluid_tab,
                       (const long*)j->file_tab, j->P, j->fluid_out, j->B, j->H, j->W, j->Ho, j->Wo, j->unroll, (long)j->nframes, aug);
    BF_CHECK_LAUNCH();
    return 0;
}
