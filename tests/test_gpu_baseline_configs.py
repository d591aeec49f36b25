"""GPU: the HIP path at the shapes BASELINE.json names (configs[0], [1], [3], [4]) -- full `film_avit_small`
(E=384, 6 heads, 12 blocks, P=16, 9 fluid parameters) with O(1)-perturbed weights, against the oracle executed on this
box's host cores on the same seeded inputs, plus size-independent properties at the full bench size.

  configs[0]  8x96x96 clip, bs 2                      -> fp32 (1e-4) and bf16 parity, forward / loss / dx / every gradient
  configs[1]  16x192x192 clip (bench shape)           -> one full-resolution sample against the oracle (bf16 tolerances) and, in fp32
                                                         and bf16, against the reference's own statistics at that size;
                                                         bs 8: bit-identical reruns, per-sample independence of the batch
  configs[3]  32x384x192 long-aspect clip (24x12 tokens, T = 32: the two-block attention paths at full width), bs 1, fp32 against the
              oracle + reference statistics, bf16 (what BASELINE names) against the reference statistics; likewise transposed
  configs[4]  bs 1 inference: the forward captured in a HIP graph replays bit-identically; 3-step rollout on device
fp32 tolerance: 1e-4 everywhere, as in tests/test_gpu_parity.py.  bf16 tolerances at FULL depth (12 blocks, E = 384): forward
<= 8e-2, dx <= 2e-1, all parameter gradients together <= 1.5e-1, each family <= 0.9.  Yardstick (measured in the build
container, configs[0] shape, same weights): the oracle itself under stock torch.autocast(bfloat16) is off by 5.2e-2 (forward),
1.3e-1 (dx), 9.0e-2 (all gradients), 1.2e-1 median / 6.4e-1 worst family against its own fp32 run -- bf16 rounding compounds
over 12 blocks with O(1) layer scales; the 3-block golden models of test_gpu_parity.py sit at 1.3e-2..2.2e-2.
"""
import pytest
import torch

from tests.helpers import fullsize_errors, rel_l2, structurally_zero

pytestmark = pytest.mark.gpu

SMALL = dict(input_fields=4, output_fields=4, patch_size=16, embed_dim=384, num_heads=6, processor_blocks=12, num_fluid_params=9)


def _inputs(B, T, H, W, seed):
    from oracle import weights as Wt
    x = Wt.synthetic_clip(B, T, 4, H, W, 100 + seed)
    y = Wt.synthetic_clip(B, T, 4, H, W, 200 + seed)
    c = Wt.synthetic_fluid_params(B, 9, 300 + seed)
    return x, y, c


def _weights(seed, cfg=None):
    from oracle import weights as Wt
    return Wt.generate(Wt.param_shapes(**(cfg or SMALL)), seed=seed)


def _oracle(B, T, H, W, seed, grads=True, dtype=torch.float32):
    """dtype = float64 for the fp32-mode comparisons: the same fp32 values evaluated in double, so that the oracle's own rounding
    (a few 1e-5 on cancellation-prone families such as FiLM's LayerNorm(9) at full depth) stays out of a 1e-4 tolerance."""
    from oracle import filmavit_ref as R
    torch.set_num_threads(16)
    sd = {k: v.to(dtype).requires_grad_(grads) for k, v in _weights(seed).items()}
    x, y, c = (t.to(dtype) for t in _inputs(B, T, H, W, seed))
    x.requires_grad_(grads)
    with torch.set_grad_enabled(grads):
        pred = R.filmavit_forward(sd, x, c, patch_size=16, num_heads=6)
        loss = R.lp_loss(pred, y)
    if not grads:
        return pred, float(loss), None, None
    loss.backward()
    return pred.detach(), float(loss), x.grad.detach(), {k: v.grad.detach() for k, v in sd.items()}


def _model(seed, dtype, T):
    from bubbleformer_amd.models import get_model
    m = get_model("filmavit", time_window=T, drop_path=0.0, compute_dtype=dtype, **SMALL)
    m.load_state_dict(_weights(seed))
    return m.cuda()


def _product(B, T, H, W, seed, dtype):
    m = _model(seed, dtype, T)
    x, y, c = (t.cuda() for t in _inputs(B, T, H, W, seed))
    x.requires_grad_(True)
    loss, pred = m.forward_loss(x, c, y)
    loss.backward()
    return pred.detach().cpu(), float(loss.detach()), x.grad.detach().cpu(), {k: p.grad.detach().cpu() for k, p in m.named_parameters()}


# bf16 throughput mode at FULL depth: every gradient family must also POINT the way the oracle's does (measured worst: 0.968 at 8x96x96 --
# blocks.3.temporal.attn_scale_factor, 6 values -- and 0.923 at 16x192x192 -- film_embed.film_net.1.weight, whose gradient passes through all 12 blocks)
BF16_FAMILY_COSINE = 0.9


def _compare(prod, orac, dtype):
    pred, loss, dx, grads = prod
    pred_o, loss_o, dx_o, grads_o = orac
    f32 = dtype == torch.float32
    ft = 1e-4 if f32 else 8e-2
    gt = 1e-4 if f32 else 1.5e-1
    assert rel_l2(pred, pred_o) < ft
    assert abs(loss - loss_o) / abs(loss_o) < ft
    assert rel_l2(dx, dx_o) < (1e-4 if f32 else 2e-1)
    num = den = 0.0
    worst_cos = (1.0, "")
    gscale = max(float(g.norm()) for g in grads_o.values())
    for k, g in grads.items():
        ref = grads_o[k]
        num += float((g.double() - ref.double()).pow(2).sum())
        den += float(ref.double().pow(2).sum())
        if structurally_zero(k):
            assert float(g.norm()) <= (1e-5 if f32 else 1e-2) * gscale, k
        else:
            assert rel_l2(g, ref) < (gt if f32 else 0.9), k
            if not f32 and float(ref.norm()) > 1e-6 * gscale:      # direction of every gradient family at full depth, not only its size
                cos = float(torch.nn.functional.cosine_similarity(g.double().flatten(), ref.double().flatten(), dim=0))
                worst_cos = min(worst_cos, (cos, k))
    if not f32:
        print("worst gradient-family cosine against the oracle", worst_cos)
        assert worst_cos[0] > BF16_FAMILY_COSINE, worst_cos
    assert (num / den) ** 0.5 < gt


def _against_reference(name, prod, dtype):
    """The same result against the REFERENCE's own fp64 run at this size, kept as statistics (tests/golden/fullsize_<name>.npz,
    SURVEY.md section 8c item 5; seeds shared with oracle/gen_golden.py: FULLSIZE).  Same tolerances as `_compare`."""
    e = fullsize_errors(name, *prod)
    f32 = dtype == torch.float32
    ft, dt, gt, fam = (1e-4, 1e-4, 1e-4, 1e-4) if f32 else (8e-2, 2e-1, 1.5e-1, 0.9)
    assert e["loss"] < ft and e["pred_samples"] < ft and e["pred_mean"] < ft and e["pred_std"] < ft and e["pred_l2"] < ft, e
    assert e["dx_samples"] < dt and e["dx_l2"] < dt, e
    assert e["grad_l2_all"] < gt and e["grad_samples"] < gt and e["grad_l2_worst"] < fam, e
    assert e["grad_zero_families"] < (1e-5 if f32 else 1e-2), e


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_config0_8x96x96_bs2(dtype):
    B, T, H, W, seed = 2, 8, 96, 96, 11
    prod = _product(B, T, H, W, seed, dtype)
    _compare(prod, _oracle(B, T, H, W, seed, dtype=torch.float64 if dtype == torch.float32 else torch.float32), dtype)
    _against_reference("config0_8x96x96_bs2", prod, dtype)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_config1_full_resolution_sample(dtype):
    B, T, H, W, seed = 1, 16, 192, 192, 12
    prod = _product(B, T, H, W, seed, dtype)
    if dtype == torch.bfloat16:
        _compare(prod, _oracle(B, T, H, W, seed), dtype)
    _against_reference("config1_16x192x192", prod, dtype)


def test_config3_long_aspect_32x384x192_fp32():
    """24 x 12 tokens, T = 32: temporal and axial-H attention take the two-block (L > 16) paths at full model width."""
    B, T, H, W, seed = 1, 32, 384, 192, 13
    prod = _product(B, T, H, W, seed, torch.float32)
    _compare(prod, _oracle(B, T, H, W, seed, dtype=torch.float64), torch.float32)
    _against_reference("config3_32x384x192", prod, torch.float32)


def test_config3_transposed_32x192x384_fp32():
    """The wide variant SURVEY.md section 8(d) asks for beside configs[3] ("stresses axial-W"): 12 x 24 tokens, so the W pass is the
    one with L = 24."""
    B, T, H, W, seed = 1, 32, 192, 384, 16
    prod = _product(B, T, H, W, seed, torch.float32)
    _compare(prod, _oracle(B, T, H, W, seed, dtype=torch.float64), torch.float32)
    _against_reference("config3_32x192x384", prod, torch.float32)


def test_config3_long_aspect_32x384x192_bf16():
    """BASELINE names configs[3] "bf16": the throughput mode at 288-token frames takes paths no other full-width test touches -- the
    two-kernel data gradient + sliced InstanceNorm backward inside the trunk (the whole-frame tile needs 144-token frames), the
    two-block (L = 24, 32) MFMA attention at d = 64 x 6 heads, the streaming GEMMs at 9,216 tokens -- against the REFERENCE's own fp64
    statistics at this size, bf16 tolerances of configs[0] / [1]."""
    B, T, H, W, seed = 1, 32, 384, 192, 13
    _against_reference("config3_32x384x192", _product(B, T, H, W, seed, torch.bfloat16), torch.bfloat16)


def test_config3_transposed_32x192x384_bf16():
    B, T, H, W, seed = 1, 32, 192, 384, 16
    _against_reference("config3_32x192x384", _product(B, T, H, W, seed, torch.bfloat16), torch.bfloat16)


def test_config1_weight_gradients_are_bit_reproducible():
    """The weight-gradient GEMMs sum token slices into slabs and add the slabs in a fixed order (gemm_tokred.hip): two backward passes
    on the same inputs give bit-identical gradients for every 1x1-conv / Linear weight and bias of the trunk (the split-K fp32 atomics
    they replace did not), a bit-identical loss and d(clip) (the fused loss adds its partial sums as 64-bit integers: float adds there
    used to flip ~12 % of every gradient tensor's bf16 elements between runs).  The remaining families (InstanceNorm / attention
    parameter partial sums, patch-embedding weights through their atomic path) are compared to rounding."""
    B, T, H, W, seed = 1, 16, 192, 192, 12
    p1 = _product(B, T, H, W, seed, torch.bfloat16)
    p2 = _product(B, T, H, W, seed, torch.bfloat16)
    assert p1[1] == p2[1] and torch.equal(p1[0], p2[0]) and torch.equal(p1[2], p2[2])
    g1, g2 = p1[3], p2[3]
    exact = ("input_head.weight", "input_head.bias", "mlp.fc1.weight", "mlp.fc1.bias", "mlp.fc2.weight", "mlp.fc2.bias")
    n_exact = 0
    for k in g1:
        if k.startswith("blocks.") and k.endswith(exact):
            assert torch.equal(g1[k], g2[k]), k
            n_exact += 1
        elif not structurally_zero(k):
            assert rel_l2(g1[k], g2[k]) < 5e-4, k          # fp32 atomics in a different order: 1.3e-4 seen on debed.out_proj.9.weight
    assert n_exact == 12 * (2 * 2 + 4)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_film_avit_big_full_depth_sample(dtype):
    """config/model_cfg/film_avit_big.yaml at FULL depth (E = 768, 12 heads, 12 blocks, 115,314,882 parameters), one 16x192x192 sample,
    against the reference's own fp64 statistics at that size (tests/golden/fullsize_big_16x192x192.npz, oracle/gen_golden.py --fullsize):
    fp32 1e-4, bf16 the full-depth bounds of configs[0] / [1]."""
    from bubbleformer_amd.models import get_model
    big = dict(SMALL, embed_dim=768, num_heads=12)
    B, T, H, W, seed = 1, 16, 192, 192, 17
    m = get_model("filmavit", time_window=T, drop_path=0.0, compute_dtype=dtype, **big)
    assert sum(p.numel() for p in m.parameters()) == 115314882
    m.load_state_dict(_weights(seed, big))
    m = m.cuda()
    x, y, c = (t.cuda() for t in _inputs(B, T, H, W, seed))
    x.requires_grad_(True)
    loss, pred = m.forward_loss(x, c, y)
    loss.backward()
    prod = (pred.detach().cpu(), float(loss.detach()), x.grad.detach().cpu(), {k: p.grad.detach().cpu() for k, p in m.named_parameters()})
    _against_reference("big_16x192x192", prod, dtype)


def test_config1_bench_size_properties():
    """bs 8 x 16x192x192, bf16, eval: reruns are bit-identical; a sample's prediction does not depend on its batch mates
    (InstanceNorm is per frame, attention per sequence) beyond bf16 GEMM tiling noise."""
    B, T, H, W, seed = 8, 16, 192, 192, 14
    m = _model(seed, torch.bfloat16, T).eval()
    x, y, c = (t.cuda() for t in _inputs(B, T, H, W, seed))
    with torch.no_grad():
        p1 = m(x, c)
        p2 = m(x, c)
        assert torch.equal(p1, p2)
        assert torch.isfinite(p1).all()
        for i in (0, 5):
            pi = m(x[i:i + 1], c[i:i + 1])
            assert rel_l2(pi[0], p1[i]) < 1e-2
        loss, _ = m.forward_loss(x, c, y)
        num = ((p1 - y) ** 2).sum(dim=(-1, -2)).sqrt()
        den = (y ** 2).sum(dim=(-1, -2)).sqrt()
        assert abs(float(loss) - float((num / den).mean(0).mean(0).sum())) < 2e-3 * float(loss)      # fused loss == LpLoss of the prediction


def test_config4_forward_in_hip_graph_and_rollout():
    """bs 1 inference (scripts/inference.py:239-252): the eval forward is capturable in a HIP graph and replays
    bit-identically; an autoregressive rollout stays on the device and matches the eager loop."""
    B, T, H, W, seed = 1, 16, 192, 192, 15
    m = _model(seed, torch.bfloat16, T).eval()
    x, _, c = (t.cuda() for t in _inputs(B, T, H, W, seed))
    with torch.no_grad():
        eager = m(x, c)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(2):
                m(x, c)
        torch.cuda.current_stream().wait_stream(s)
        static_x = x.clone()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            static_out = m(static_x, c)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(static_out, eager)
        # rollout: feed the prediction back (graph replay vs eager)
        cur = x.clone()
        for _ in range(3):
            static_x.copy_(cur)
            g.replay()
            cur = static_out.clone()
        ref = x.clone()
        for _ in range(3):
            ref = m(ref, c)
        assert torch.isfinite(cur).all()
        assert torch.equal(cur, ref)


@pytest.mark.parametrize("B", [1, 2])
def test_config4_inference_trunk_equals_the_stage_forwards(B, monkeypatch):
    """bs 1 inference takes the whole-trunk inference path (bf_trunk_eval_fwd: whole-frame projection kernels with the InstanceNorms
    inside, weights prepared once): the prediction equals the stage-by-stage forward BIT FOR BIT (statistics are summed in
    bf_in_stats' order, products in bf_gemm's), follows a parameter update (torch in-place op and this package's optimizer kernel),
    and matches the oracle at the bf16 full-depth bound."""
    import ctypes, json
    from bubbleformer_amd import _lib as L, ops
    T, H, W, seed = 16, 192, 192, 15
    m = _model(seed, torch.bfloat16, T).eval()
    x, _, c = (t.cuda() for t in _inputs(B, T, H, W, seed))
    h = L.lib()
    with torch.no_grad():
        h.bf_prof_enable(1)
        fast = m(x, c)
        torch.cuda.synchronize()
        buf = ctypes.create_string_buffer(1 << 14)
        h.bf_prof_report(buf, len(buf))
        h.bf_prof_enable(0)
        names = json.loads(buf.value.decode())
        assert any(k.startswith("frame_linear") for k in names) and not any(k.startswith("in_stats") and names[k]["calls"] > 12 for k in names), names.keys()
        monkeypatch.setenv("BF_TRUNK_EVAL", "0")
        slow = m(x, c)
        monkeypatch.delenv("BF_TRUNK_EVAL")
        assert torch.equal(fast, slow), "fraction of differing elements: %g" % float((fast != slow).float().mean())
        if B == 1:
            pred_o, _, _, _ = _oracle(B, T, H, W, seed, grads=False)
            assert rel_l2(fast.cpu(), pred_o) < 8e-2
        # the prepared weights follow the parameters
        p = m.blocks[3].spatial.mlp.fc1.weight
        p.mul_(1.5)
        f2 = m(x, c)
        monkeypatch.setenv("BF_TRUNK_EVAL", "0")
        s2 = m(x, c)
        monkeypatch.delenv("BF_TRUNK_EVAL")
        assert torch.equal(f2, s2) and not torch.equal(f2, fast)
        q = m.blocks[5].temporal.output_head.weight
        ops.adamw_(q.view(-1), torch.ones_like(q).view(-1), torch.zeros_like(q).view(-1), torch.zeros_like(q).view(-1), 1, 0.05)
        f3 = m(x, c)
        monkeypatch.setenv("BF_TRUNK_EVAL", "0")
        s3 = m(x, c)
        assert torch.equal(f3, s3) and not torch.equal(f3, f2)


def test_config1_chained_stage_heads_change_no_bit(monkeypatch):
    """bf_stage_chain_next: a stage's opening InstanceNorm computed by the last GEMM launch of the stage in front of it (the temporal
    out-projection for the axial block, fc2 + MLP-branch norm for the next temporal block: one launch and one read of the activation less each)
    gives the prediction, the loss, d(clip) and every deterministic gradient family bit for bit as the unchained calls do; and the chained
    launches really replace 23 statistics launches of the 12-block trunk."""
    import ctypes, json
    from bubbleformer_amd import _lib as L
    B, T, H, W, seed = 1, 16, 192, 192, 12
    h = L.lib()

    def run():
        h.bf_prof_enable(1)
        prod = _product(B, T, H, W, seed, torch.bfloat16)
        torch.cuda.synchronize()
        buf = ctypes.create_string_buffer(1 << 15)
        h.bf_prof_report(buf, len(buf))
        h.bf_prof_enable(0)
        return prod, json.loads(buf.value.decode())["in_stats"]["calls"]

    p1, n1 = run()
    monkeypatch.setenv("BF_STAGE_CHAIN", "0")
    p2, n2 = run()
    # chained: only the temporal norm2 (12) and block 0's opening norm are launches of their own; unchained: + 12 spatial norm1 + 11 temporal norm1
    # (the MLP-branch norm sits in the fc2 launch either way: bf_gemm_fwd_frames)
    assert n2 - n1 == 23, (n1, n2)
    assert p1[1] == p2[1] and torch.equal(p1[0], p2[0]) and torch.equal(p1[2], p2[2])
    exact = ("input_head.weight", "input_head.bias", "mlp.fc1.weight", "mlp.fc1.bias", "mlp.fc2.weight", "mlp.fc2.bias")
    for k in p1[3]:
        if k.startswith("blocks.") and k.endswith(exact):
            assert torch.equal(p1[3][k], p2[3][k]), k


def test_config1_backward_chain_matches_the_separate_norm_backward(monkeypatch):
    """bf_stage_chain_tail inside a TrainStep (deferred side work, the only mode it arms in): the temporal stage's last kernel also applies the
    backward of the spatial stage's MLP-branch InstanceNorm in front of it.  Against the same step with the chains off: same loss bit
    for bit (the forward chain changes no bit), gradients equal to rounding (the frame sums of the chained norm are taken in another order
    and on fp32-in-register rows), and the launch profile shows 11 chained kernels and 11 statistics-backward launches less."""
    import ctypes, json
    from bubbleformer_amd import _lib as L
    from bubbleformer_amd.trainer import TrainStep
    B, T, H, W, seed = 2, 16, 192, 192, 12
    h = L.lib()
    x, y, c = (t.cuda() for t in _inputs(B, T, H, W, seed))

    def run():
        m = _model(seed, torch.bfloat16, T)       # (drop_path = 0: the two runs see the same network)
        step = TrainStep(m, lr=0.0, weight_decay=0.0)
        h.bf_prof_enable(1)
        loss = float(step(x, c, y))
        torch.cuda.synchronize()
        buf = ctypes.create_string_buffer(1 << 15)
        h.bf_prof_report(buf, len(buf))
        h.bf_prof_enable(0)
        return loss, step.flat.grad.detach().clone(), json.loads(buf.value.decode())

    l1, g1, n1 = run()
    monkeypatch.setenv("BF_STAGE_CHAIN", "0")
    l2, g2, n2 = run()
    assert n1.get("gemm_pair<inbwd,chain>", {}).get("calls", 0) == 11, sorted(n1)
    assert n2["in_bwd"]["calls"] - n1["in_bwd"]["calls"] == 11
    assert l1 == l2
    assert float((g1 - g2).norm()) < 2e-3 * float(g2.norm())


def test_config1_backward_chain_under_stochastic_depth(monkeypatch):
    """With drop_path = 0.2 (the bench's setting) and the same random draw in both runs the chained norm takes the per-frame table of the MLP
    branch (gtab = drop[f] * gamma): same loss, gradients equal to rounding."""
    import ctypes, json
    from bubbleformer_amd import _lib as L
    from bubbleformer_amd.models import get_model
    from bubbleformer_amd.trainer import TrainStep
    B, T, H, W, seed = 2, 16, 192, 192, 12
    h = L.lib()
    x, y, c = (t.cuda() for t in _inputs(B, T, H, W, seed))

    def run():
        m = get_model("filmavit", time_window=T, drop_path=0.2, compute_dtype=torch.bfloat16, **SMALL)
        m.load_state_dict(_weights(seed))
        m = m.cuda().train()
        step = TrainStep(m, lr=0.0, weight_decay=0.0)
        torch.manual_seed(77)
        h.bf_prof_enable(1)
        loss = float(step(x, c, y))
        torch.cuda.synchronize()
        buf = ctypes.create_string_buffer(1 << 15)
        h.bf_prof_report(buf, len(buf))
        h.bf_prof_enable(0)
        return loss, step.flat.grad.detach().clone(), json.loads(buf.value.decode())

    l1, g1, n1 = run()
    monkeypatch.setenv("BF_STAGE_CHAIN", "0")
    l2, g2, n2 = run()
    assert n1.get("gemm_pair<inbwd,chain>", {}).get("calls", 0) == 11 and "gemm_pair<inbwd,chain>" not in n2, sorted(n1)
    assert l1 == l2
    assert float((g1 - g2).norm()) < 2e-3 * float(g2.norm())


def test_config1_training_step_takes_the_streaming_embed_debed_kernels():
    """A bf16 training step at the configs[1] clip size runs the round-3 kernels at the two ends of the model, not their generic fallbacks:
    the library's own launch profile names the one-pass embed tail, the last-debed backward passes, the gather / scatter stage GEMMs and
    the gather weight gradients, and no sliced InstanceNorm backward touches a full-resolution map (what remains is the 48 x 48 and
    24 x 24 maps: 2 phases x 4 norms)."""
    import ctypes, json
    from bubbleformer_amd import _lib as L
    B, T, H, W, seed = 1, 16, 192, 192, 12
    m = _model(seed, torch.bfloat16, T)
    x, y, c = (t.cuda() for t in _inputs(B, T, H, W, seed))
    h = L.lib()
    h.bf_prof_enable(1)
    loss, _ = m.forward_loss(x, c, y)
    loss.backward()
    torch.cuda.synchronize()
    buf = ctypes.create_string_buffer(1 << 15)
    h.bf_prof_report(buf, len(buf))
    h.bf_prof_enable(0)
    names = json.loads(buf.value.decode())
    for k in ("embed_tail_bwd", "debed_last_bwd<stats>", "debed_last_bwd<apply>", "gather_gemm<gelu>", "gather_gemm<gelu,rebuilt>", "gather_gemm<plain>",
              "scatter_gemm<gelu>", "scatter_gemm<plain>", "gather_wgrad<fine gelu>", "gather_wgrad<fine gelu,rebuilt>", "gather_wgrad<coarse gelu>"):
        assert k in names, (k, sorted(names))
    # the first embed stage's 226 MB map is not stored: the stage behind it and its weight gradient rebuild its rows from the patch rows
    assert names["gather_gemm<gelu,rebuilt>"]["calls"] == 1 and names["gather_gemm<gelu>"]["calls"] == 1 and names["scatter_gemm<gelu>"]["calls"] == 2
    assert names["gather_wgrad<fine gelu,rebuilt>"]["calls"] == 1 and names["gather_wgrad<fine gelu>"]["calls"] == 1 and names["gather_wgrad<coarse gelu>"]["calls"] == 2


def test_inference_operators_are_registered_with_the_dispatcher():
    """torch.ops.bubbleformer_amd.trunk_eval / frame_linear (torch_ops.py): schema + fake-tensor implementation pass torch.library.opcheck,
    the eval forward shows up under its operator name in the profiler, and the model's prediction goes through it."""
    from bubbleformer_amd import torch_ops  # noqa: F401
    from bubbleformer_amd.models import get_model
    torch.manual_seed(5)
    m = get_model("filmavit", input_fields=4, output_fields=4, time_window=4, patch_size=16, embed_dim=384, num_heads=6, processor_blocks=2,
                  num_fluid_params=9, drop_path=0.0, compute_dtype=torch.bfloat16).cuda().eval()
    x, c = torch.randn(1, 4, 4, 192, 192, device="cuda"), torch.randn(1, 9, device="cuda")
    kinds, params = [], []
    for blk in m.blocks:
        kinds += [0, 1]
        params += list(blk.temporal.stage_params()) + list(blk.spatial.stage_params())
    with torch.no_grad():
        tok = m.embed.tokens(x, c, m.film_embed.film_params(), compute_dtype=torch.bfloat16)
        args = (tok, 6, True, True, kinds, [p.detach() if p is not None else None for p in params])
        torch.library.opcheck(torch.ops.bubbleformer_amd.trunk_eval.default, args, test_utils=("test_schema", "test_faketensor"))
        a = torch.randn(2 * 144, 384, device="cuda").bfloat16()
        w = (torch.randn(96, 384, device="cuda") * 0.1).bfloat16()
        torch.library.opcheck(torch.ops.bubbleformer_amd.frame_linear.default, (a, w, 2, 144),
                              dict(norm_w=torch.ones(384, device="cuda"), norm_b=torch.zeros(384, device="cuda"), bias=torch.randn(96, device="cuda")),
                              test_utils=("test_schema", "test_faketensor"))
        with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CPU]) as prof:
            pred = m(x, c)
        assert any("bubbleformer_amd::trunk_eval" in e.key for e in prof.key_averages())
        assert torch.equal(m.debed.from_tokens(torch.ops.bubbleformer_amd.trunk_eval(*args)), pred)


@pytest.mark.parametrize("name,kw", [("avit", dict(attn_scale=False, feat_scale=False)), ("avit", dict(attn_scale=True, feat_scale=False)),
                                     ("filmavit", dict(attn_scale=False, feat_scale=True, num_fluid_params=9))])
def test_inference_trunk_variants_equal_the_stage_forwards(name, kw, monkeypatch):
    """The inference path with the reference's switches off (`attn_scale`, `feat_scale`: models/axial_vit.py constructor arguments) and for
    the unconditioned AViT: 3 blocks at E = 384, 4 x 192 x 192 clips, batch 2 -- bit-identical to the stage forwards."""
    from bubbleformer_amd.models import get_model
    torch.manual_seed(3)
    m = get_model(name, input_fields=4, output_fields=4, time_window=4, patch_size=16, embed_dim=384, num_heads=6, processor_blocks=3,
                  drop_path=0.1, compute_dtype=torch.bfloat16, **kw).cuda().eval()
    with torch.no_grad():
        for p in m.parameters():          # layer scales start at 1e-6: give every branch weight
            if p.ndim == 1 and float(p.abs().max()) < 1e-3:
                p.fill_(0.3)
    x = torch.randn(2, 4, 4, 192, 192, device="cuda")
    args = (x, torch.randn(2, 9, device="cuda")) if name == "filmavit" else (x,)
    with torch.no_grad():
        fast = m(*args)
        monkeypatch.setenv("BF_TRUNK_EVAL", "0")
        slow = m(*args)
    assert torch.isfinite(fast).all() and torch.equal(fast, slow)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_film_avit_big_width(dtype):
    """`film_avit_big` width (E = 768, 12 heads of 64; config/model_cfg/film_avit_big.yaml) through the same kernels: 3 blocks,
    8x64x64 clips, bs 2.  E/4 = 192 intermediate channels: 768-column patch rows, two frames x 768 channels in a prologue table.
    fp32: 1e-4.  bf16: forward 6e-2, dx 1.5e-1, all gradients 1e-1, family 0.7 -- the autocast yardstick at this shape (16-token
    frames) is 3.1e-2 / 7.5e-2 / 3.6e-2 / worst family 3.1e-1, and this path also keeps the residual stream in bf16."""
    from bubbleformer_amd.models import get_model
    from oracle import filmavit_ref as R
    big = dict(SMALL, embed_dim=768, num_heads=12, processor_blocks=3)
    B, T, H, W, seed = 2, 8, 64, 64, 16
    torch.set_num_threads(16)
    x, y, c = _inputs(B, T, H, W, seed)
    sd = {k: v.requires_grad_(True) for k, v in _weights(seed, big).items()}
    xo = x.clone().requires_grad_(True)
    pred_o = R.filmavit_forward(sd, xo, c, patch_size=16, num_heads=12)
    loss_o = R.lp_loss(pred_o, y)
    loss_o.backward()
    m = get_model("filmavit", time_window=T, drop_path=0.0, compute_dtype=dtype, **big)
    m.load_state_dict(_weights(seed, big))
    m = m.cuda()
    xg = x.cuda().requires_grad_(True)
    loss, pred = m.forward_loss(xg, c.cuda(), y.cuda())
    loss.backward()
    f32 = dtype == torch.float32
    assert rel_l2(pred.detach().cpu(), pred_o.detach()) < (1e-4 if f32 else 6e-2)
    assert rel_l2(xg.grad.cpu(), xo.grad) < (1e-4 if f32 else 1.5e-1)
    num = den = 0.0
    for k, p in m.named_parameters():
        ref = sd[k].grad
        num += float((p.grad.cpu().double() - ref.double()).pow(2).sum())
        den += float(ref.double().pow(2).sum())
        if not structurally_zero(k):
            assert rel_l2(p.grad.cpu(), ref) < (1e-4 if f32 else 0.7), k
    assert (num / den) ** 0.5 < (1e-4 if f32 else 1e-1)


SWEEP = [
    # B, T, H,  W,  patch, E,   heads, film
    (1, 1, 16, 16, 4, 64, 2, True),        # single frame: temporal attention over one token
    (1, 3, 8, 40, 4, 32, 1, True),         # h = 2, w = 10, one head of 32
    (2, 5, 48, 16, 8, 128, 1, True),       # head dim 128, patch 8
    (3, 2, 64, 32, 16, 192, 6, False),     # AViT (no FiLM), 6 heads of 32
    (1, 17, 8, 8, 2, 96, 3, True),         # T = 17 (two-block temporal attention), patch 2, 4x4 tokens
    (2, 4, 32, 96, 4, 64, 2, True),        # w = 24 (two-block axial-W), 8 x 24 tokens = 192 per frame (register-cache edge)
    (1, 2, 56, 60, 4, 72, 3, True),        # 14 x 15 = 210 tokens per frame (> 192: sliced statistics in the trunk), E = 72 (E/4 = 18 channels)
    (5, 1, 4, 4, 4, 32, 4, True),          # one token per frame, head dim 8
]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("B,T,H,W,patch,E,heads,film", SWEEP)
def test_shape_sweep(B, T, H, W, patch, E, heads, film, dtype):
    """Odd shapes against the fp64 oracle, fp32 mode (1e-4) and bf16 mode (6e-2 forward, 1.5e-1 dx and all gradients, families 0.7): single tokens / frames,
    non-square and non-power-of-two token grids, every supported head dimension, frames on both sides of the 192-token
    register-cache boundary, all patch sizes.  Shapes whose head dim or E/4 is not a whole number of 16-byte chunks must be refused."""
    from bubbleformer_amd.models import get_model
    from oracle import filmavit_ref as R, weights as Wt
    cfg = dict(input_fields=3, output_fields=2, patch_size=patch, embed_dim=E, num_heads=heads, processor_blocks=2)
    if film:
        cfg["num_fluid_params"] = 5
    ch = 4 if dtype == torch.float32 else 8
    ok_dims = (E // heads) % ch == 0 and (E // 4) % ch == 0
    seed = 40 + B + T + H
    sd0 = Wt.generate(Wt.param_shapes(**cfg), seed=seed)
    x = Wt.synthetic_clip(B, T, 3, H, W, 100 + seed)
    y = Wt.synthetic_clip(B, T, 2, H, W, 200 + seed)
    c = Wt.synthetic_fluid_params(B, 5, 300 + seed)
    m = get_model("filmavit" if film else "avit", time_window=T, drop_path=0.0, compute_dtype=dtype, **cfg)
    m.load_state_dict(sd0)
    m = m.cuda()
    xg = x.cuda().requires_grad_(True)
    args = (xg, c.cuda()) if film else (xg,)
    if not ok_dims:
        with pytest.raises(Exception):
            m.forward_loss(*args, y.cuda())
        return
    loss, pred = m.forward_loss(*args, y.cuda())
    loss.backward()
    od = torch.float64
    sd = {k: v.to(od).requires_grad_(True) for k, v in sd0.items()}
    xo = x.to(od).requires_grad_(True)
    kw = dict(patch_size=patch, num_heads=heads)
    pred_o = R.filmavit_forward(sd, xo, c.to(od), **kw) if film else R.avit_forward(sd, xo, **kw)
    lo = R.lp_loss(pred_o, y.to(od))
    lo.backward()
    f32 = dtype == torch.float32
    ft, gt = (1e-4, 1e-4) if f32 else (6e-2, 1.5e-1)     # bf16: the same code is exact to 1e-4 in fp32 mode; observed 1.5e-2 .. 4.5e-2 forward
    assert rel_l2(pred.detach().cpu(), pred_o.detach()) < ft
    assert abs(float(loss.detach()) - float(lo.detach())) / abs(float(lo.detach())) < ft
    assert rel_l2(xg.grad.cpu(), xo.grad) < (gt if f32 else 1.5e-1)
    num = den = 0.0
    gscale = max(float(v.grad.norm()) for v in sd.values())
    for k, p in m.named_parameters():
        ref = sd[k].grad
        num += float((p.grad.cpu().double() - ref).pow(2).sum())
        den += float(ref.pow(2).sum())
        if structurally_zero(k) or float(ref.norm()) < 1e-7 * gscale:
            assert float((p.grad.cpu().double() - ref).norm()) <= (2e-5 if f32 else 1e-2) * gscale, k
        else:
            err = float((p.grad.cpu().double() - ref).norm())
            # bf16: a family passes on its own norm, or (rounding-noise families such as FiLM's LayerNorm bias, whose gradient is a
            # near-cancelling sum) on the scale of the largest family
            noisy = k.startswith("film_embed.film_net.0.")      # LayerNorm(P) of the fluid parameters: sums of 2E near-cancelling terms
            assert err < (2e-4 if f32 else 0.7) * float(ref.norm()) or (not f32 and err < (5e-2 if noisy else 5e-3) * gscale), k
    assert (num / den) ** 0.5 < gt


def test_graph_survives_a_larger_problem_and_follows_weight_updates():
    """A HIP graph holds the raw addresses of the scratch arena and of the prepared-weights arena it was captured with.  Both are pinned:
    capture at batch 1, run a batch-8 forward + a training-shaped forward/backward (a larger arena request), replay -- the replay equals
    the eager forward bit for bit.  And a GraphedForward kept across a parameter update replays with the NEW weights (the arena is
    re-prepared in place before the replay)."""
    from bubbleformer_amd import ops
    from bubbleformer_amd.utils.rollout import GraphedForward
    T, H, W, seed = 16, 192, 192, 21
    m = _model(seed, torch.bfloat16, T).eval()
    x1, _, c1 = (t.cuda() for t in _inputs(1, T, H, W, seed))
    x8, y8, c8 = (t.cuda() for t in _inputs(8, T, H, W, seed + 1))
    with torch.no_grad():
        eager1 = m(x1, c1)
        fwd = GraphedForward(m, x1, c1)
        assert torch.equal(fwd(x1), eager1)
        big = m(x8, c8)                                   # more frames than the whole-frame path takes: stage forwards, larger scratch
        assert torch.isfinite(big).all()
    m.train()
    loss, _ = m.forward_loss(x8, c8, y8)                  # and a backward (the largest arena of all)
    loss.backward()
    m.eval()
    torch.cuda.synchronize()
    with torch.no_grad():
        assert torch.equal(fwd(x1), eager1), "replay after a larger problem differs from the eager forward"
        # weights change under the captured graph
        m.blocks[2].spatial.mlp.fc2.weight.mul_(1.25)
        q = m.blocks[7].temporal.input_head.weight
        ops.adamw_(q.view(-1), torch.ones_like(q).view(-1), torch.zeros_like(q).view(-1), torch.zeros_like(q).view(-1), 1, 0.02)
        replayed = fwd(x1).clone()
        eager2 = m(x1, c1)
        assert torch.equal(replayed, eager2) and not torch.equal(replayed, eager1)
    assert len(ops._SCRATCH_PINNED) >= 1


def test_frame_linear_and_trunk_eval_reject_malformed_operands():
    """The dispatcher-visible operators validate what the kernels would otherwise read or write out of bounds through raw pointers."""
    from bubbleformer_amd import _lib as L, torch_ops  # noqa: F401
    E = L.BubbleformerHipError
    dt = torch.bfloat16
    a = torch.randn(2 * 144, 384, device="cuda").to(dt)
    w = torch.randn(768, 384, device="cuda").to(dt)
    op = torch.ops.bubbleformer_amd.frame_linear
    assert op(a, w, 2, 144).shape == (288, 768)
    with pytest.raises(E):
        op(a, w, 3, 144)                                               # frames * tokens != rows
    with pytest.raises(E):
        op(a, w[:, :256].contiguous(), 2, 144)                         # K mismatch
    with pytest.raises(E):
        op(a.float(), w, 2, 144)                                       # dtype
    with pytest.raises(E):
        op(a, w, 2, 144, bias=torch.zeros(100, device="cuda"))         # table shorter than N
    with pytest.raises(E):
        op(a, w, 2, 144, bias=torch.zeros(768, device="cuda", dtype=dt))     # table dtype
    with pytest.raises(E):
        op(a, w, 2, 144, resid=torch.zeros(288, 384, device="cuda", dtype=dt))       # residual shape
    with pytest.raises(E):
        op(a, w, 2, 144, norm_w=torch.ones(384, device="cuda"))        # half a pair
    with pytest.raises(E):
        op(a[:, ::2], w[:, ::2], 2, 144)                               # inner stride
    m = _model(3, dt, 16).eval()
    blk = m.blocks[0]
    params = list(blk.temporal.stage_params()) + list(blk.spatial.stage_params())
    tok = torch.randn(1, 16, 12, 12, 384, device="cuda").to(dt)
    te = torch.ops.bubbleformer_amd.trunk_eval
    assert te(tok, 6, True, True, [0, 1], params).shape == tok.shape
    bad = list(params)
    bad[6] = bad[6][:100]                                              # a truncated input_head.weight
    with pytest.raises(E):
        te(tok, 6, True, True, [0, 1], bad)
    with pytest.raises(E):
        te(tok, 5, True, True, [0, 1], params)                         # 384 is not a multiple of 5 heads
    with pytest.raises(E):
        te(tok, 6, True, True, [0, 1], params[:-1])                    # list does not match the kinds


def test_config1_batch8_backward_matches_the_single_sample_fixture():
    """The bench's own launch geometry (batch 8: M = 18,432 tokens, twelve token slices x 6-8 tiles in the weight-gradient kernel, 72 row
    tiles in the streaming GEMMs) against the REFERENCE's fp64 statistics of one 16x192x192 sample (fullsize_config1): the loss means
    over the batch (utils/losses.py:60-65), so a batch of eight copies of that sample has the sample's loss and parameter gradients, and
    d(clip) of every copy is 1/8 of the sample's.  fp32 mode at the 1e-4 bound, bf16 at the full-depth bf16 bounds."""
    T, H, W, seed = 16, 192, 192, 12
    for dtype in (torch.float32, torch.bfloat16):
        m = _model(seed, dtype, T)
        x, y, c = (t.cuda() for t in _inputs(1, T, H, W, seed))
        x8 = x.repeat(8, 1, 1, 1, 1).requires_grad_(True)
        loss, pred = m.forward_loss(x8, c.repeat(8, 1), y.repeat(8, 1, 1, 1, 1))
        loss.backward()
        dx = x8.grad.detach()
        for i in (1, 7):                                   # every copy sees the same numbers (rows of different tiles / slices)
            assert rel_l2(pred[i], pred[0]) < (1e-6 if dtype == torch.float32 else 2e-2)
            assert rel_l2(dx[i], dx[0]) < (1e-5 if dtype == torch.float32 else 5e-2)
        prod = (pred[3:4].detach().cpu(), float(loss.detach()), (8.0 * dx[3:4]).cpu(), {k: p.grad.detach().cpu() for k, p in m.named_parameters()})
        _against_reference("config1_16x192x192", prod, dtype)
        del m, x8, loss, pred, dx
        torch.cuda.empty_cache()


def test_training_step_at_384_frames_takes_the_stored_map_path():
    """A per-GPU batch of 24 clips of 16 frames at 192 x 192 (F = 384): the one-pass embed backward tail's partials no longer fit the
    token-reduction workspace (F <= 367 at this geometry), so the forward must NOT drop the stage-0 map (the "lean" embed) -- before the
    backward's limits were part of that decision such a step failed in bf_embed_bwd.  A 2-block bf16 model without an input gradient
    (the training case); the embed's gradients against the same step at F = 96 frames four times over (same clips, batch-mean loss)."""
    from bubbleformer_amd.models import get_model
    T, H, W, seed = 16, 192, 192, 12
    cfg = dict(SMALL, processor_blocks=2)
    x, y, c = (t.cuda() for t in _inputs(6, T, H, W, seed))

    def run(rep):
        torch.manual_seed(0)
        m = get_model("filmavit", time_window=T, drop_path=0.0, compute_dtype=torch.bfloat16, **cfg)
        m.load_state_dict(_weights(seed, cfg))
        m = m.cuda()
        loss, _ = m.forward_loss(x.repeat(rep, 1, 1, 1, 1), c.repeat(rep, 1), y.repeat(rep, 1, 1, 1, 1))
        loss.backward()
        torch.cuda.synchronize()
        return float(loss.detach()), {k: p.grad.detach().clone() for k, p in m.named_parameters()}

    l4, g4 = run(4)          # 24 clips: F = 384
    l1, g1 = run(1)          # 6 clips: F = 96 (the lean path)
    assert abs(l4 - l1) < 2e-3 * abs(l1)
    for k in g1:
        if k.startswith("embed.") and not structurally_zero(k):
            assert torch.isfinite(g4[k]).all(), k
            assert rel_l2(g4[k], g1[k]) < 6e-2, (k, rel_l2(g4[k], g1[k]))


def test_native_trunk_call_and_folded_slab_sums_change_no_bit(monkeypatch):
    """(1) ops.trunk_train (bf_trunk_train_fwd / bwd: the 24 stage calls, chain hints and gradient-ready callbacks from C++) against the
    per-stage Python path (BF_TRUNK_NATIVE=0): the same kernels in the same order, so loss, d(clip) and EVERY gradient bit for bit --
    in a TrainStep (deferred side work, chained tails, direct gradient slots).  (2) The weight-gradient slab sums riding in the next
    token-reduction launch (bf_gemm_tokred_deferred) against a launch of their own each (bf_debug_tokred_fold(0)): slice order is the
    same, so every weight gradient bit for bit."""
    from bubbleformer_amd import _lib as L
    from bubbleformer_amd.models import get_model
    from bubbleformer_amd.trainer import TrainStep
    B, T, H, W, seed = 2, 16, 192, 192, 12
    x, y, c = (t.cuda() for t in _inputs(B, T, H, W, seed))

    def run():
        torch.manual_seed(3)      # the same stochastic-depth draw in every run
        m = get_model("filmavit", time_window=T, drop_path=0.2, compute_dtype=torch.bfloat16, **SMALL)
        m.load_state_dict(_weights(seed))
        m = m.cuda().train()
        step = TrainStep(m, lr=0.0, weight_decay=0.0)
        loss = float(step(x, c, y))
        torch.cuda.synchronize()
        return loss, step.flat.grad.detach().clone()

    exact = ("input_head.weight", "input_head.bias", "output_head.weight", "mlp.fc1.weight", "mlp.fc1.bias", "mlp.fc2.weight", "mlp.fc2.bias")
    l1, g1 = run()
    l1b, g1b = run()
    monkeypatch.setenv("BF_TRUNK_NATIVE", "0")
    l2, g2 = run()
    monkeypatch.delenv("BF_TRUNK_NATIVE")
    L.lib().bf_debug_tokred_fold(0)
    try:
        l3, g3 = run()
    finally:
        L.lib().bf_debug_tokred_fold(1)
    assert l1 == l1b == l2 == l3
    # float atomics (norm / attention parameter sums) make a few small tensors order dependent run to run: compare what is deterministic
    noise = float((g1 - g1b).abs().max())
    assert float((g1 - g2).abs().max()) <= max(noise, 1e-30) * 4 + 1e-12
    assert float((g1 - g3).abs().max()) <= max(noise, 1e-30) * 4 + 1e-12
    m = get_model("filmavit", time_window=T, drop_path=0.2, compute_dtype=torch.bfloat16, **SMALL)
    off = 0
    for k, p in m.named_parameters():
        n = (p.numel() + 63) // 64 * 64
        if k.startswith("blocks.") and k.endswith(exact):
            a = g1[off:off + p.numel()]
            assert torch.equal(a, g2[off:off + p.numel()]) and torch.equal(a, g3[off:off + p.numel()]), k
        off += n


def test_training_step_is_bit_reproducible_run_to_run():
    """Two identical bf16 training steps at the bench geometry (16 x 192 x 192, stochastic depth on, the deferred two-queue backward the
    trainer uses): the loss AND every one of the parameter gradients come out with the same bits.  Nothing in the step adds floats in
    arrival order any more: weight gradients are slab sums in slice order (gemm_tokred.hip, bf_gemm_slabs), the small parameter
    reductions have one writer per value (param_reduce.h), the loss is an integer sum.  (Round 4 found this the hard way: the check
    exposed a kernel whose result was not merely re-ordered but WRONG by 1e-4 .. 1e-2 in one channel block: tokred_narrow.  The fault
    followed one packed fp32 instruction form (v_pk_fma_f32 with op_sel on the low lane, two workgroups on a CU), not the prologue
    loads first suspected; its root cause is open -- EXPERIMENTS.md round 4 -- and the build's register audit refuses the form.)"""
    from bubbleformer_amd import ops
    from bubbleformer_amd.models import get_model

    def grads():
        torch.manual_seed(5)
        m = get_model("filmavit", time_window=16, drop_path=0.2, compute_dtype=torch.bfloat16, **dict(SMALL, processor_blocks=4)).cuda().train()
        x, y, c = (t.cuda() for t in _inputs(2, 16, 192, 192, 21))
        torch.manual_seed(9)                     # the stochastic-depth draws
        ops.set_side_defer(True)
        try:
            loss, _ = m.forward_loss(x, c, y)
            loss.backward()
        finally:
            ops.set_side_defer(False)
        torch.cuda.synchronize()
        return float(loss), {k: p.grad.detach().clone() for k, p in m.named_parameters()}

    l1, g1 = grads()
    l2, g2 = grads()
    assert l1 == l2
    differing = [k for k in g1 if not torch.equal(g1[k], g2[k])]
    assert not differing, differing


def test_pending_parameter_reduction_is_flushed_on_the_stream_that_made_it():
    """The library's call-to-call record is per device, its scratch arenas per (device, stream).  One bf16 axial stage, forward and backward
    on stream A in deferred mode with direct gradient slots: nothing joins at the end of the stage, so its InstanceNorm / attention
    parameter reductions stay pending (no temporal stage follows to carry them).  `set_side_defer(False)` under stream B then has to launch
    them: on A, behind the kernels that wrote their partial sums, with B waiting for that -- after a synchronise of B alone every
    parameter gradient equals, bit for bit, the same calls made on one stream."""
    from bubbleformer_amd import _lib as L, ops
    dt, T = torch.bfloat16, 16
    blk = _model(3, dt, T).train().blocks[0].spatial
    params = list(blk.stage_params())
    torch.manual_seed(4)
    tok = torch.randn(2, T, 12, 12, 384, device="cuda").to(dt)
    dout = torch.randn_like(tok)
    da, dm = ops.drop_path_factors(2 * T, 0.2, tok.device), ops.drop_path_factors(2 * T, 0.2, tok.device)
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()

    def run(join_stream):
        slots = {p.data_ptr(): torch.zeros_like(p) for p in params if p is not None}
        torch.cuda.synchronize()
        ops.set_direct_grad_slots(slots)
        try:
            with torch.cuda.stream(sa):
                ops.set_side_defer(True)
                ops.spatial_block(tok, 6, True, True, params, da, dm).backward(dout)
            with torch.cuda.stream(join_stream):
                ops.set_side_defer(False)
                got = [None if p is None else slots[p.data_ptr()].clone() for p in params]
            join_stream.synchronize()
        finally:
            ops.set_side_defer(False)
            ops.set_direct_grad_slots(None)
            torch.cuda.synchronize()
        return got

    one, two = run(sa), run(sb)
    assert float(one[L.SPATIAL_FIELDS.index("norm1_w")].abs().max()) > 0      # (a gradient the pending reduction writes)
    differing = [n for n, a, b in zip(L.SPATIAL_FIELDS, one, two) if a is not None and not torch.equal(a, b)]
    assert not differing, differing
