"""CPU: the C-ABI library builds for gfx950, loads, and exports every symbol include/bubbleformer_hip.h declares;
the product path refuses to run without a GPU (no CPU fallback)."""
import os
import re

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    txt = open(os.path.join(REPO, "include", "bubbleformer_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(bf_[a-z0-9_]+)\s*\(", txt)))


def test_library_exports_every_declared_symbol():
    from bubbleformer_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    h = _lib.lib()
    names = _declared()
    assert len(names) >= 30
    for n in names:
        assert hasattr(h, n), n
    assert set(names) == set(_lib.SIGNATURES), set(names) ^ set(_lib.SIGNATURES)
    assert h.bf_abi_version() == 3


RECORDS = {"bf_rollout_step": "RolloutStep", "bf_census_rows": "CensusRows", "bf_link_rows": "LinkRows", "bf_error_rows": "ErrorRows",
           "bf_ensemble_rows": "EnsembleRows", "bf_opt_step": "OptStep"}


def _record_fields(name):
    """[(field, ctypes type)] of `typedef struct name { ... } name;` as the header declares it: any pointer is a c_void_p, int64_t a c_int64,
    int32_t / int a c_int32, float a c_float; a declaration may name several fields (`float *a, *b;`, the star belongs to the declarator)."""
    import ctypes as C
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "bubbleformer_hip.h")).read(), flags=re.S)
    m = re.search(r"typedef\s+struct\s+%s\s*\{(.*?)\}\s*%s\s*;" % (name, name), txt, flags=re.S)
    assert m, name
    scalars = {"int64_t": C.c_int64, "int32_t": C.c_int32, "int": C.c_int32, "float": C.c_float}
    fields = []
    for decl in filter(None, (d.strip() for d in m.group(1).split(";"))):
        base, rest = re.match(r"(?:const\s+)?(\w+)\s*(.*)$", decl, flags=re.S).groups()
        for d in rest.split(","):
            fields.append((d.replace("*", "").strip(), C.c_void_p if "*" in d else scalars[base]))
    return fields


@pytest.mark.parametrize("name", sorted(RECORDS))
def test_record_mirrors_the_header(name):
    """A ctypes record has the header's fields under the header's names, in its order and of its types, and neither has padding: two fields
    of one type in the wrong order are a different list of names, which the positional argument lists could not show."""
    import ctypes as C
    from bubbleformer_amd import _lib
    rec = getattr(_lib, RECORDS[name])
    declared = _record_fields(name)
    assert [(n, t) for n, t in rec._fields_] == declared
    assert C.sizeof(rec) == sum(C.sizeof(t) for _, t in declared)


_OPT_BUF = []


def _opt_step(**kw):
    """A bf_opt_step every check accepts -- 16-byte aligned host buffers nothing reads, a coefficient, an average and one parameter group --
    with `kw` over it; the value "+4" (or "+2") puts a pointer 4 (2) bytes past its valid place."""
    import ctypes as C
    from bubbleformer_amd import _lib as L
    if not _OPT_BUF:
        _OPT_BUF.append((C.c_char * 144)())
    p = (C.addressof(_OPT_BUF[0]) + 15) // 16 * 16
    good = dict(p=p, g=p + 16, m=p + 32, v=p + 48, coef_dev=p + 64, avg=p + 80, chunk_group=p + 96, group_lr_scale=p + 100, group_weight_decay=p + 104,
                group_frozen=p + 108, n=4, step=1, n_groups=1, lr=1e-3, beta1=0.9, beta2=0.99, eps=1e-8, wd=0.0, gscale=1.0, clip_value=float("inf"),
                avg_weight=0.5)
    return L.OptStep(**{**good, **{k: good[k] + int(v) if v in ("+4", "+2") else v for k, v in kw.items()}})


# defect -> (the fields it sets, what the refusal says); bf_lion reads neither step nor v, so those three are the Adams' alone
_OPT_DEFECTS = {
    "n_zero": (dict(n=0), "n must be positive"), "step_zero": (dict(step=0), "step must be >= 1"), "v_null": (dict(v=None), "null pointer"),
    "p_off_by_4": (dict(p="+4"), "buffers must be 16-byte aligned"), "g_off_by_4": (dict(g="+4"), "buffers must be 16-byte aligned"),
    "m_off_by_4": (dict(m="+4"), "buffers must be 16-byte aligned"), "v_off_by_4": (dict(v="+4"), "buffers must be 16-byte aligned"),
    "clip_zero": (dict(clip_value=0.0), "clip_value must be positive"), "clip_negative": (dict(clip_value=-1.0), "clip_value must be positive"),
    "clip_nan": (dict(clip_value=float("nan")), "clip_value must be positive"),
    "avg_weight_zero": (dict(avg_weight=0.0), "avg_weight must be in (0, 1]"), "avg_weight_1.5": (dict(avg_weight=1.5), "avg_weight must be in (0, 1]"),
    "avg_weight_nan": (dict(avg_weight=float("nan")), "avg_weight must be in (0, 1]"),
    "avg_off_by_4": (dict(avg="+4"), "the average buffer must be 16-byte aligned"),
    "lr_scale_null": (dict(group_lr_scale=None), "a chunk map needs the three group tables"), "weight_decay_null": (dict(group_weight_decay=None), "a chunk map needs the three group tables"),
    "frozen_null": (dict(group_frozen=None), "a chunk map needs the three group tables"),
    "lr_scale_off_by_2": (dict(group_lr_scale="+2"), "the group tables must be 4-byte aligned"),
    "weight_decay_off_by_2": (dict(group_weight_decay="+2"), "the group tables must be 4-byte aligned"),
    "n_groups_zero": (dict(n_groups=0), "n_groups must be 1 .. 64"), "n_groups_65": (dict(n_groups=65), "n_groups must be 1 .. 64"),
}
_OPT_CASES = [(name, d) for name in ("bf_adamw", "bf_adam", "bf_lion") for d in sorted(_OPT_DEFECTS)
              if not (name == "bf_lion" and d in ("step_zero", "v_null", "v_off_by_4"))]


@pytest.mark.parametrize("name,defect", _OPT_CASES)
def test_optimizer_record_with_one_defect_is_refused(name, defect):
    """bf_adamw / bf_adam / bf_lion run every check of their record before any HIP call: no GPU needed.  An otherwise valid record (host
    buffers nobody reads) with exactly one defect is refused under the entry's name and for that defect; no valid call is made here."""
    import ctypes as C
    from bubbleformer_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    h = _lib.lib()
    fields, reason = _OPT_DEFECTS[defect]
    assert getattr(h, name)(C.byref(_opt_step(**fields)), None) != 0
    assert (name + ": " + reason) in h.bf_last_error().decode(), h.bf_last_error()


def _null_pointer_calls():
    """name -> (call with every record NULL, call with full records whose first required pointer alone is NULL); every other pointer is the
    address of a host buffer nothing reads, every size valid.  bf_field_errors' record has no required member: there it is `pred`."""
    import ctypes as C
    from bubbleformer_amd import _lib as L
    buf = (C.c_char * 64)()
    p = C.addressof(buf)

    def step(**kw):
        return L.RolloutStep(**{**dict(pred=p, frames=p, field_stride=64, total_frames=4, first=p, step=p, field=p, diff=p, div=p, nfields=1, B=1, T=2,
                                       C=1, H=4, W=4, Ho=4, Wo=4, steps=1), **kw})

    def census(**kw):
        return L.CensusRows(**{**dict(count=p, cells=p, attached=p, area=p), **kw})

    links = L.LinkRows(*[p] * 6)
    errs, ref = L.ErrorRows(), C.byref
    opt = lambda name: lambda h, s: getattr(h, name)(s and ref(_opt_step(p=None)), None)      # noqa: E731
    return {
        "bf_adamw": opt("bf_adamw"), "bf_adam": opt("bf_adam"), "bf_lion": opt("bf_lion"),
        "bf_rollout_score": lambda h, s: h.bf_rollout_score(s and ref(step(pred=None)), -1, 1.0, p, p, None, None, None, None, p, 1 << 20, None),
        "bf_rollout_heatflux": lambda h, s: h.bf_rollout_heatflux(s and ref(step(pred=None)), 0, 0, p, 0.0, 1.0, 1.0, 1.0, p, p, None),
        "bf_rollout_bubbles": lambda h, s: h.bf_rollout_bubbles(s and ref(step(pred=None)), 0, 4, 1, s and ref(census()), s and ref(census()), None, p, 1 << 20, None),
        "bf_rollout_bubble_links": lambda h, s: h.bf_rollout_bubble_links(s and ref(step(pred=None)), 1, p, s and ref(census()), s and ref(census()),
                                                                          s and ref(links), s and ref(links), p, 1 << 20, None),
        "bf_rollout_errors": lambda h, s: h.bf_rollout_errors(s and ref(step(pred=None)), -1, 1, 0, 0, 0, s and ref(errs), p, 1 << 20, None),
        "bf_bubble_links": lambda h, s: h.bf_bubble_links(p, s and ref(census(count=None)), 1, 2, 4, 4, 1, s and ref(links), p, 1 << 20, None),
        "bf_field_errors": lambda h, s: h.bf_field_errors(p if not s else None, p, None, 1, 4, 4, 1, 0, 0, 0, s and ref(errs), p, 1 << 20, None),
    }


@pytest.mark.parametrize("name", ["bf_rollout_score", "bf_rollout_heatflux", "bf_rollout_bubbles", "bf_rollout_bubble_links", "bf_rollout_errors",
                                  "bf_bubble_links", "bf_field_errors", "bf_adamw", "bf_adam", "bf_lion"])
def test_null_record_and_null_member_are_refused(name):
    """Each re-signed entry point refuses a NULL record, and a record whose first required pointer is NULL, as its null pointer: both return at
    the first check, before any HIP call, so no GPU is needed."""
    from bubbleformer_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    h = _lib.lib()
    call = _null_pointer_calls()[name]
    for with_records in (None, True):
        assert call(h, with_records) != 0
        assert h.bf_last_error().decode().endswith(name + ": null pointer"), (with_records, h.bf_last_error())


def test_register_audit_no_spills_beside_counted_waits():
    """tools/register_audit.py over the compiler's per-kernel resource remarks of the in-tree build: no kernel compiled from a source file
    with hand-counted `s_waitcnt vmcnt` waits (ring / pair / stream / token-reduction GEMM families) may spill or use scratch."""
    from bubbleformer_amd import _lib
    from tools import register_audit
    if not os.path.isdir(register_audit.BUILD) or not any(f.endswith(".remarks") for f in os.listdir(register_audit.BUILD)):
        _lib.build()
    rows, bad, warn, missing = register_audit.audit()
    assert not missing, missing
    assert len(rows) > 100 and sum(1 for k in rows if k["counted_waits"]) >= 30
    assert {"gemm_pair_kernel<0>", "gemm_pair_kernel<1>", "gemm_pair_kernel<2>", "tokred_pp_kernel<3>"} <= {k["kernel"] for k in rows}
    assert not bad, [(k["kernel"], k.get("vgpr_spill"), k.get("scratch")) for k in bad]


def test_register_audit_counted_set_survives_the_shared_header(tmp_path):
    """The counted-wait helpers live in csrc/lane_ops.h, so a file that orders memory by count may hold no `s_waitcnt` text of its own:
    counted_wait_files() knows the helpers by call name.  The set is the one the files' local copies used to give -- the LDS-DMA GEMM
    families, and the two label kernels whose global passes drain by `s_waitcnt vmcnt(0)` (drain_and_sync)."""
    from tools import register_audit
    assert register_audit.counted_wait_files() == {"frame_fwd", "gemm_frame", "gemm_stream", "gemm_tokred", "bubbles", "bubble_tracks"}
    (tmp_path / "calls.hip").write_text('#include "lane_ops.h"\n__global__ void k(int n) { wait_vm_n(3); }\n')
    (tmp_path / "drains.hip").write_text('#include "lane_ops.h"\n__global__ void k() { drain_and_sync(); }\n')
    (tmp_path / "gemm_like.hip").write_text('#include "gemm_common.h"\n__global__ void k() { __syncthreads(); }\n')      # the include alone does not count
    (tmp_path / "lane_ops.h").write_text(open(os.path.join(register_audit.CSRC, "lane_ops.h")).read())
    assert register_audit.counted_wait_files(str(tmp_path)) == {"calls", "drains"}


def test_no_cpu_fallback():
    from bubbleformer_amd import _lib
    from bubbleformer_amd.models import get_model
    m = get_model("filmavit", input_fields=4, output_fields=4, time_window=2, patch_size=4, embed_dim=64, num_heads=1,
                  processor_blocks=1, drop_path=0.0, num_fluid_params=9)
    with pytest.raises(_lib.BubbleformerHipError):
        m(torch.randn(1, 2, 4, 8, 8), torch.randn(1, 9))


def test_registry_contract():
    from bubbleformer_amd.models import get_model, list_models, register_model
    assert list_models() == ["avit", "filmavit"]
    with pytest.raises(KeyError):
        get_model("nope")
    with pytest.raises(ValueError):
        register_model("avit")(object)


def test_state_dict_matches_reference_inventory():
    from bubbleformer_amd.models import get_model
    from oracle import weights as W
    cfg = dict(input_fields=4, output_fields=4, patch_size=16, embed_dim=384, num_heads=6, processor_blocks=12, num_fluid_params=9)
    m = get_model("filmavit", time_window=16, drop_path=0.0, **cfg)
    shapes = W.param_shapes(**cfg)
    sd = m.state_dict()
    assert list(sd.keys()) == list(shapes.keys()) and len(sd) == 506
    assert sum(v.numel() for v in sd.values()) == 28906602
    assert all(tuple(sd[k].shape) == tuple(shapes[k]) for k in shapes)


def test_register_audit_flags_compiler_loads_inside_a_counted_dma_loop(tmp_path):
    """The second build-time rule (tools/register_audit.py: foreign_loads): a load hipcc issued itself inside the innermost loop that
    orders LDS-DMA by a hand-counted `s_waitcnt vmcnt(N)` fails the build; the same load in an enclosing loop's own blocks does not
    (the shape of tokred_narrow_kernel<.., true> before and after the round-4 fix)."""
    from tools import register_audit
    dma = ";;#ASMSTART\n\tglobal_load_lds_dwordx4 v[18:19], off\n;;#ASMEND\n"
    wait = ";;#ASMSTART\n\ts_waitcnt vmcnt(7)\n;;#ASMEND\n"
    bad = ("_Z3badv:                                ; @_Z3badv\n.LBB0_1:                                ; =>This Inner Loop Header: Depth=1\n"
           "\tglobal_load_dword v2, v[22:23], off\n" + dma + wait + "\ts_cbranch_vccnz .LBB0_1\n.Lfunc_end0:\n")
    good = ("_Z4goodv:                               ; @_Z4goodv\n.LBB1_1:                                ; =>This Loop Header: Depth=1\n"
            "\tglobal_load_dword v2, v[22:23], off\n;;#ASMSTART\n\ts_waitcnt vmcnt(0)\n;;#ASMEND\n"
            ".LBB1_2:                                ;   Parent Loop BB1_1 Depth=1\n                                        ; =>  This Inner Loop Header: Depth=2\n"
            + dma + wait + "\ts_cbranch_vccnz .LBB1_2\n; %bb.3:                                ;   in Loop: Header=BB1_1 Depth=1\n\ts_cbranch_vccnz .LBB1_1\n.Lfunc_end1:\n")
    f = tmp_path / "k.s"
    f.write_text(bad + good)
    nested_bad = ("_Z6nestedv:                             ; @_Z6nestedv\n.LBB2_1:                                ; =>This Loop Header: Depth=1\n"
                  ".LBB2_2:                                ;   Parent Loop BB2_1 Depth=1\n                                        ; =>  This Inner Loop Header: Depth=2\n"
                  "\tglobal_load_dword v2, v[22:23], off\n" + dma + wait + "\ts_cbranch_vccnz .LBB2_2\n\ts_cbranch_vccnz .LBB2_1\n.Lfunc_end2:\n")
    f.write_text(bad + good + nested_bad)
    hits = register_audit.foreign_loads(str(f))
    assert [k for k, _ in hits] == ["_Z3badv", "_Z6nestedv"], hits


def test_register_audit_flags_packed_fp32_ops_with_the_low_lane_on_a_high_half(tmp_path):
    """The third build-time rule (tools/register_audit.py: packed_high_select): `v_pk_fma_f32 .. op_sel:[0,1,1]` (low lane from the high
    registers of src1 / src2) fails the build -- the form measured wrong in tokred_narrow_kernel<6, true> (EXPERIMENTS.md, round 4);
    the default selectors, the high-lane selectors and a src0 swap do not."""
    from tools import register_audit
    f = tmp_path / "k.s"
    f.write_text("_Z3badv:                                ; @_Z3badv\n\tv_pk_fma_f32 v[26:27], v[26:27], v[2:3], v[8:9] op_sel:[0,1,1]\n.Lfunc_end0:\n"
                 "_Z4bad2v:                               ; @_Z4bad2v\n\tv_pk_mul_f32 v[26:27], v[26:27], v[2:3] op_sel:[0,1]\n.Lfunc_end1:\n"
                 "_Z4goodv:                               ; @_Z4goodv\n\tv_pk_fma_f32 v[34:35], v[22:23], v[2:3], v[8:9] op_sel_hi:[1,0,0]\n"
                 "\tv_pk_fma_f32 v[136:137], v[150:151], v[220:221], v[136:137] op_sel:[1,0,0] op_sel_hi:[0,1,1]\n\tv_pk_fma_f32 v[2:3], v[4:5], v[6:7], v[8:9]\n.Lfunc_end2:\n")
    assert [k for k, _ in register_audit.packed_high_select(str(f))] == ["_Z3badv", "_Z4bad2v"]
