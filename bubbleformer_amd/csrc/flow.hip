// Flow consistency of a signed-distance field phi and a velocity (u, v): do the fields of ONE prediction agree with each other?  The reference has
// no program for this; DESIGN.md section 32 has the definitions and include/bubbleformer_hip.h the contract.  Frames [H][W] fp32, x along W, y
// along H, spacing dx on both axes, vapour iff phi > 0; interior cells 1 <= y <= H - 2, 1 <= x <= W - 2.  Per frame:
//   divergence_rms   sqrt(mean over the bulk cells of div^2), div = ((u[y][x+1] - u[y][x-1]) + (v[y+1][x] - v[y-1][x])) / (2 dx); a bulk cell is an
//                    interior cell whose (2 r + 1)^2 window (clipped to the frame) holds no vapour cell; bulk_cells their number;
//   kinetic_energy   mean over all cells of (u^2 + v^2) / 2;
//   enstrophy        mean over the interior cells of w^2 / 2, w = ((v[y][x+1] - v[y][x-1]) - (u[y+1][x] - u[y-1][x])) / (2 dx).
// Per pair of consecutive frames (0 the earlier, 1 the later), with the means pm = (phi0 + phi1) / 2, um, vm and s = (phi1 - phi0) / dt:
//   transport_rms        sqrt(mean over the band cells of (s + um d/dx pm + vm d/dy pm)^2), central differences; a band cell is an interior cell
//                        with |pm| < band; transport_cells their number;
//   interface_speed_rms  sqrt(mean over the band cells of s^2).
//
// One workgroup of 1024 threads owns a frame: its frame rows and the pair that ends in it, so no two workgroups exchange data inside a launch
// (the rollout's carry has two halves for that reason).  The stencils read their neighbours from global memory: a frame's three fields are a few
// hundred KB that one workgroup walks in raster order, so the neighbour reads are served by the CU's L1 and the L2.  Every value is widened to
// fp64 before any arithmetic; a thread adds its cells in raster order and the workgroup's sums go through bf_common.h's block_reduce, so two calls
// give the same bits and a frame has the same bits alone and in a batch.  No workspace, no atomics.
#include "clip_store.h"

namespace {
constexpr int NT = 1024;
constexpr int NW = NT / 64;
constexpr int FLOW_MIN_SIDE = 3, FLOW_MAX_SIDE = 1024;

// one field of one frame on the model's grid: p[nearest_src(y) * ld + nearest_src(x)], de-normalised or not, widened
struct Field {
    const float* p; int ld, Hs, Ws; float sy, sx; bool ident, denorm; float q, d;
    __device__ __forceinline__ double at(int y, int x) const {
        const float v = p[(long)nearest_src(y, sy, Hs, ident) * ld + nearest_src(x, sx, Ws, ident)];
        return (double)(denorm ? denormalise(v, q, d) : v);
    }
};
struct Frame { Field phi, u, v; };

__device__ __forceinline__ Field plain_field(const float* p, int H, int W) { return Field{p, W, H, W, 1.f, 1.f, true, false, 1.f, 0.f}; }

// where a frame's rows go: the element of every output, or null
struct FlowOut { float *div, *ke, *ens; int32_t* bulk; float *tr, *sp; int32_t* tcells; };

__device__ __forceinline__ FlowOut out_at(const bf_flow_rows& r, long frame_row, long pair_row, bool has_pair) {
    return FlowOut{r.divergence_rms ? r.divergence_rms + frame_row : nullptr, r.kinetic_energy ? r.kinetic_energy + frame_row : nullptr,
                   r.enstrophy ? r.enstrophy + frame_row : nullptr, r.bulk_cells ? r.bulk_cells + frame_row : nullptr,
                   has_pair && r.transport_rms ? r.transport_rms + pair_row : nullptr,
                   has_pair && r.interface_speed_rms ? r.interface_speed_rms + pair_row : nullptr,
                   has_pair && r.transport_cells ? r.transport_cells + pair_row : nullptr};
}

// the rows of frame c and, with has_e, of the pair (e, c); keep (optional, [3][H W]) receives c's (phi, u, v) as the kernel read them
__device__ __forceinline__ void flow_frame(const Frame& c, const Frame& e, bool has_e, int H, int W, float dx, float dt, float band_f, int r,
                                           const FlowOut& o, float* keep) {
    __shared__ double red[NW];
    const int n = H * W, tid = threadIdx.x;
    const double inv_2dx = 1.0 / (2.0 * (double)dx), inv_dt = 1.0 / (double)dt, band = (double)band_f;
    const bool want_div = o.div || o.bulk, want_ke = o.ke != nullptr, want_ens = o.ens != nullptr;
    const bool want_pair = has_e && (o.tr || o.sp || o.tcells);
    double a_div = 0.0, a_bulk = 0.0, a_ke = 0.0, a_ens = 0.0, a_tr = 0.0, a_sp = 0.0, a_band = 0.0;
    for (int i = tid; i < n; i += NT) {
        const int y = i / W, x = i - y * W;
        if (want_ke || keep) {
            const double uc = c.u.at(y, x), vc = c.v.at(y, x);
            if (want_ke) a_ke += 0.5 * (uc * uc + vc * vc);
            if (keep) { keep[i] = (float)c.phi.at(y, x); keep[n + i] = (float)uc; keep[2 * n + i] = (float)vc; }
        }
        if (y < 1 || y > H - 2 || x < 1 || x > W - 2) continue;
        if (want_ens) {
            const double w = ((c.v.at(y, x + 1) - c.v.at(y, x - 1)) - (c.u.at(y + 1, x) - c.u.at(y - 1, x))) * inv_2dx;
            a_ens += 0.5 * (w * w);
        }
        if (want_div) {
            bool vapour = false;
            for (int yy = max(y - r, 0); yy <= min(y + r, H - 1) && !vapour; ++yy)
                for (int xx = max(x - r, 0); xx <= min(x + r, W - 1); ++xx) vapour |= c.phi.at(yy, xx) > 0.0;      // false for a NaN and an exact zero
            if (!vapour) {
                const double dv = ((c.u.at(y, x + 1) - c.u.at(y, x - 1)) + (c.v.at(y + 1, x) - c.v.at(y - 1, x))) * inv_2dx;
                a_div += dv * dv;
                a_bulk += 1.0;
            }
        }
        if (want_pair) {
            const double p0 = e.phi.at(y, x), p1 = c.phi.at(y, x), pm = 0.5 * (p0 + p1);
            if (fabs(pm) < band) {                                          // false for a NaN
                const double s = (p1 - p0) * inv_dt;
                const double um = 0.5 * (e.u.at(y, x) + c.u.at(y, x)), vm = 0.5 * (e.v.at(y, x) + c.v.at(y, x));
                const double px = (0.5 * (e.phi.at(y, x + 1) + c.phi.at(y, x + 1)) - 0.5 * (e.phi.at(y, x - 1) + c.phi.at(y, x - 1))) * inv_2dx;
                const double py = (0.5 * (e.phi.at(y + 1, x) + c.phi.at(y + 1, x)) - 0.5 * (e.phi.at(y - 1, x) + c.phi.at(y - 1, x))) * inv_2dx;
                const double res = s + um * px + vm * py;
                a_tr += res * res;
                a_sp += s * s;
                a_band += 1.0;
            }
        }
    }
    // the flags are the same in every thread of the workgroup: each reduction is reached by all or by none.  The counts are sums of ones, exact in fp64
    if (want_ke) {
        const double t = block_reduce<RED_SUM, NW>(a_ke, red);
        if (tid == 0) *o.ke = (float)(t / ((double)H * (double)W));
    }
    if (want_ens) {
        const double t = block_reduce<RED_SUM, NW>(a_ens, red);
        if (tid == 0) *o.ens = (float)(t / ((double)(H - 2) * (double)(W - 2)));
    }
    if (want_div) {
        const double t = block_reduce<RED_SUM, NW>(a_div, red), cells = block_reduce<RED_SUM, NW>(a_bulk, red);
        if (tid == 0) {
            if (o.div) *o.div = (float)sqrt(t / cells);                      // 0 / 0: NaN without a bulk cell
            if (o.bulk) *o.bulk = (int32_t)cells;
        }
    }
    if (want_pair) {
        const double cells = block_reduce<RED_SUM, NW>(a_band, red);
        if (o.tr) {
            const double t = block_reduce<RED_SUM, NW>(a_tr, red);
            if (tid == 0) *o.tr = (float)sqrt(t / cells);
        }
        if (o.sp) {
            const double t = block_reduce<RED_SUM, NW>(a_sp, red);
            if (tid == 0) *o.sp = (float)sqrt(t / cells);
        }
        if (o.tcells && tid == 0) *o.tcells = (int32_t)cells;
    }
}

struct FlowArgs { const float *sdf, *velx, *vely; int T, H, W; float dx, dt, band; int r; bf_flow_rows rows; };

__global__ void __launch_bounds__(NT) flow_kernel(FlowArgs a) {
    const long f = blockIdx.x, n = (long)a.H * a.W;
    const int t = (int)(f % a.T);
    const long seq = f / a.T;
    const Frame c{plain_field(a.sdf + f * n, a.H, a.W), plain_field(a.velx + f * n, a.H, a.W), plain_field(a.vely + f * n, a.H, a.W)};
    const long fe = t > 0 ? f - 1 : f;                                     // the earlier frame of the pair that ends here; unread at t = 0
    const Frame e{plain_field(a.sdf + fe * n, a.H, a.W), plain_field(a.velx + fe * n, a.H, a.W), plain_field(a.vely + fe * n, a.H, a.W)};
    flow_frame(c, e, t > 0, a.H, a.W, a.dx, a.dt, a.band, a.r, out_at(a.rows, f, seq * (a.T - 1) + t - 1, t > 0), nullptr);
}

struct RolloutFlowArgs { RolloutStep v; int ch[3]; float dx, dt, band; int r; float* carry; bf_flow_rows rows[2]; };

// the three channels of prediction frame bt in physical units, of the stored frame fr on the model's grid, and of a carry slot
__device__ __forceinline__ Frame predicted_frame(const RolloutFlowArgs& a, long bt) {
    const RolloutStep& v = a.v;
    auto field = [&](int c) { return Field{v.predicted(bt, c), v.Wo, v.Ho, v.Wo, 1.f, 1.f, true, true, v.dv[c], v.diff[c]}; };
    return Frame{field(a.ch[0]), field(a.ch[1]), field(a.ch[2])};
}
__device__ __forceinline__ Frame stored_frame(const RolloutFlowArgs& a, long fr) {
    const RolloutStep& v = a.v;
    auto field = [&](int c) { return Field{v.stored(c, fr), v.W, v.H, v.W, v.sy(), v.sx(), v.ident(), false, 1.f, 0.f}; };
    return Frame{field(a.ch[0]), field(a.ch[1]), field(a.ch[2])};
}
__device__ __forceinline__ float* carry_slot(const RolloutFlowArgs& a, int half, int b) {
    return a.carry + ((long)half * a.v.B + b) * 3 * ((long)a.v.Ho * a.v.Wo);
}

// workgroup = (side, trajectory, frame): side 0 the prediction, side 1 the simulation
__global__ void __launch_bounds__(NT) rollout_flow_kernel(RolloutFlowArgs a) {
    const RolloutStep& v = a.v;
    const int s = v.current();
    if (s < 0) return;                                                     // behind the last row: nothing is written, the carry included
    const int BT = v.B * v.T, side = blockIdx.x / BT, bt = blockIdx.x % BT, t = bt % v.T, b = bt / v.T;
    const long n = (long)v.Ho * v.Wo;
    const bool has_pair = t > 0 || s > 0;                                  // the pair from the last input frame to the first predicted one is not scored
    Frame c, e;
    float* keep = nullptr;
    if (side == 0) {
        c = predicted_frame(a, bt);
        if (t > 0) e = predicted_frame(a, bt - 1);
        else if (s > 0) {
            const float* k = carry_slot(a, (s - 1) & 1, b);
            e = Frame{plain_field(k, v.Ho, v.Wo), plain_field(k + n, v.Ho, v.Wo), plain_field(k + 2 * n, v.Ho, v.Wo)};
        }
        if (t == v.T - 1) keep = carry_slot(a, s & 1, b);
    } else {
        c = stored_frame(a, v.frame(s, b, t));
        if (has_pair) e = stored_frame(a, v.frame(s, b, t - 1));           // t = 0: the last frame of the step before, first[b] + (s + 1) T - 1
    }
    const long pair_row = (long)b * ((long)v.steps * v.T - 1) + (long)s * v.T + t - 1;
    flow_frame(c, e, has_pair, v.Ho, v.Wo, a.dx, a.dt, a.band, a.r, out_at(a.rows[side], v.row(s, b, t), pair_row, has_pair), keep);
}

bool side_ok(int n) { return n >= FLOW_MIN_SIDE && n <= FLOW_MAX_SIDE; }
}  // namespace

extern "C" int bf_flow_consistency(const float* sdf, const float* velx, const float* vely, int64_t sequences, int T, int H, int W, float dx, float dt,
                                   float band, int interface_radius, const bf_flow_rows* rows, bf_stream_t stream) {
    BF_REQUIRE(rows && sdf && velx && vely, "bf_flow_consistency: null pointer");
    BF_REQUIRE(side_ok(H) && side_ok(W), "bf_flow_consistency: H and W must lie in [3, 1024]");
    BF_REQUIRE(sequences > 0 && T > 0 && sequences <= 0x7fffffff / T, "bf_flow_consistency: bad sizes");
    BF_REQUIRE(dx > 0.f && dt > 0.f && band > 0.f && interface_radius >= 1, "bf_flow_consistency: dx, dt and band must be positive, interface_radius >= 1");
    const FlowArgs a{sdf, velx, vely, T, H, W, dx, dt, band, interface_radius, *rows};
    hipLaunchKernelGGL(flow_kernel, dim3((unsigned)(sequences * T)), dim3(NT), 0, (hipStream_t)stream, a);
    BF_CHECK_LAUNCH();
    return 0;
}

extern "C" int bf_rollout_flow(const bf_rollout_step* s, int sdf_channel, int velx_channel, int vely_channel, float dx, float dt, float band,
                               int interface_radius, float* carry, const bf_flow_rows* pred, const bf_flow_rows* target, bf_stream_t stream) {
    RolloutStep v;
    if (const int rc = rollout_step_view(v, s, carry && pred && target, s && (int64_t)s->B * s->T <= 0x3fffffff, "bf_rollout_flow: null pointer",
                                         "bf_rollout_flow: bad sizes"))
        return rc;
    BF_REQUIRE(side_ok(v.Ho) && side_ok(v.Wo), "bf_rollout_flow: Ho and Wo must lie in [3, 1024]");
    BF_REQUIRE(sdf_channel >= 0 && sdf_channel < v.C && velx_channel >= 0 && velx_channel < v.C && vely_channel >= 0 && vely_channel < v.C,
               "bf_rollout_flow: the signed-distance and velocity channels must be output channels");
    BF_REQUIRE(dx > 0.f && dt > 0.f && band > 0.f && interface_radius >= 1, "bf_rollout_flow: dx, dt and band must be positive, interface_radius >= 1");
    const RolloutFlowArgs a{v, {sdf_channel, velx_channel, vely_channel}, dx, dt, band, interface_radius, carry, {*pred, *target}};
    hipLaunchKernelGGL(rollout_flow_kernel, dim3((unsigned)(2 * v.B * v.T)), dim3(NT), 0, (hipStream_t)stream, a);
    BF_CHECK_LAUNCH();
    return 0;
}
