// Seeded Gaussian noise on a batch of clips: dst[b][t][c][y][x] = fmaf(sigma[c], z, src[b][t][c][y][x]) on contiguous fp32 (B, T, C, H, W).
// z is a pure function of (seed, sample id, draw, pass, element index inside the sample's clip) -- a counter-based generator, no state, so
// a sample gets the same noise in any batch, at any batch position, launch geometry or world size, and a resumed run continues the sequence.
//   generator  Philox4x32-10 (Random123's constants), key = the 64-bit seed, low word first
//   counter    {g, sample id (low 32 bits), draw, pass} for elements 4g .. 4g + 3 of the sample's flattened (T, C, H, W) clip
//   normals    Box-Muller per word pair (a, b): u1 = ((a >> 8) + 1) 2^-24 in (0, 1], u2 = (b >> 8) 2^-24 in [0, 1), r = sqrtf(-2 logf(u1)),
//              the pair r cospif(2 u2), r sinpif(2 u2) (2 u2 is exact: no rounded 2 pi); words (0, 1) -> elements 4g, 4g + 1, words (2, 3) ->
//              4g + 2, 4g + 3; |z| <= sqrt(48 ln 2) = 5.77.  The accurate library functions, never the approximate ones.
// A streaming kernel: one thread per group of four elements, grid-stride over a sample's groups, samples on the grid's y axis; 16-byte loads
// and stores when the per-sample size is a multiple of 4 and both pointers are 16-byte aligned, scalar ones otherwise (clip_store.hip's
// split).  No LDS, no atomics; dst == src (in place) is allowed, a partial overlap is not.
#include "philox.h"
#include <algorithm>

namespace {
constexpr int NT = 256;
__device__ __forceinline__ void box_muller(uint32_t a, uint32_t b, float& z0, float& z1) {
    const float u1 = (float)((a >> 8) + 1u) * 0x1p-24f;      // (0, 1]: the integer is <= 2^24, exact in fp32
    const float two_u2 = (float)(b >> 8) * 0x1p-23f;         // 2 u2 in [0, 2), exact
    const float r = sqrtf(-2.0f * logf(u1));
    z0 = r * cospif(two_u2);
    z1 = r * sinpif(two_u2);
}
// sigma == 0 hands the element back untouched (fmaf(0, z, -0.0f) would be +0.0f)
__device__ __forceinline__ float perturb(float x, float s, float z) { return s == 0.0f ? x : fmaf(s, z, x); }

// VEC: n % 4 == 0 and both pointers 16-byte aligned.  n = T C H W elements per sample (< 2^31), hw = H W.
template <bool VEC>
__global__ void __launch_bounds__(NT) clip_noise_kernel(const float* src, float* dst, const float* __restrict__ sigma,
                                                       const long* __restrict__ sample_ids, uint32_t k0, uint32_t k1, uint32_t draw, uint32_t pass,
                                                       int B, int C, uint32_t hw, uint32_t n) {
    const uint32_t groups = (n + 3u) >> 2;
    for (int b = blockIdx.y; b < B; b += gridDim.y) {
        const uint32_t id = sample_ids ? (uint32_t)(unsigned long)sample_ids[b] : (uint32_t)b;
        const float* s = src + (long)b * n;
        float* d = dst + (long)b * n;
        for (uint32_t g = blockIdx.x * NT + threadIdx.x; g < groups; g += gridDim.x * NT) {
            const Quad q = philox4x32_10(g, id, draw, pass, k0, k1);
            float z[4];
            box_muller(q.w[0], q.w[1], z[0], z[1]);
            box_muller(q.w[2], q.w[3], z[2], z[3]);
            const uint32_t e = 4u * g;
            if (VEC && (hw & 3u) == 0u) {                      // the four elements lie in one frame of one channel
                const float sg = sigma[(e / hw) % (uint32_t)C];
                const float4 v = *reinterpret_cast<const float4*>(s + e);
                *reinterpret_cast<float4*>(d + e) = make_float4(perturb(v.x, sg, z[0]), perturb(v.y, sg, z[1]), perturb(v.z, sg, z[2]), perturb(v.w, sg, z[3]));
            } else if (VEC) {
                const float4 v = *reinterpret_cast<const float4*>(s + e);
                const float x[4] = {v.x, v.y, v.z, v.w};
                float o[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) o[j] = perturb(x[j], sigma[((e + j) / hw) % (uint32_t)C], z[j]);
                *reinterpret_cast<float4*>(d + e) = make_float4(o[0], o[1], o[2], o[3]);
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (e + j < n) d[e + j] = perturb(s[e + j], sigma[((e + j) / hw) % (uint32_t)C], z[j]);      // a ragged last group uses its leading words
            }
        }
    }
}
}  // namespace

extern "C" int bf_clip_noise(const float* src, float* dst, const float* sigma, const int64_t* sample_ids, uint64_t seed, uint32_t draw, uint32_t pass,
                             int B, int T, int C, int H, int W, bf_stream_t stream) {
    BF_REQUIRE(src && dst && sigma, "bf_clip_noise: null pointer");
    BF_REQUIRE(B > 0 && T > 0 && C > 0 && H > 0 && W > 0, "bf_clip_noise: bad sizes");
    const int64_t n = (int64_t)T * C * H * W;
    BF_REQUIRE(n < (1LL << 31), "bf_clip_noise: a sample's clip must hold fewer than 2^31 elements");
    BF_REQUIRE(((uintptr_t)src % 4 == 0) && ((uintptr_t)dst % 4 == 0), "bf_clip_noise: buffers must be 4-byte aligned");
    const bool vec = (n % 4 == 0) && ((uintptr_t)src % 16 == 0) && ((uintptr_t)dst % 16 == 0);
    const long groups = (n + 3) / 4;
    const int gy = std::min(B, 65535);
    const int gx = (int)std::max<long>(1, std::min<long>((groups + NT - 1) / NT, std::max(1, 256 * 16 / gy)));
    const hipStream_t st = (hipStream_t)stream;
    BfProfScope prof(st, "clip_noise", 0.0, 8.0 * (double)B * (double)n);
    const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    if (vec)
        hipLaunchKernelGGL(clip_noise_kernel<true>, dim3(gx, gy), dim3(NT), 0, st, src, dst, sigma, (const long*)sample_ids, k0, k1, draw, pass, B, C,
                           (uint32_t)(H * W), (uint32_t)n);
    else
        hipLaunchKernelGGL(clip_noise_kernel<false>, dim3(gx, gy), dim3(NT), 0, st, src, dst, sigma, (const long*)sample_ids, k0, k1, draw, pass, B, C,
                           (uint32_t)(H * W), (uint32_t)n);
    BF_CHECK_LAUNCH();
    return 0;
}
