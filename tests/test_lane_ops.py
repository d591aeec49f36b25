"""csrc/lane_ops.h holds the one definition of every lane, LDS-transpose, LDS-DMA and wait-count primitive the kernel files share: a copy
left (or grown back) in a .hip file could drift from it without any build error.  The same holds for the ordered workgroup reduction
(bf_common.h), the LDS transform with its radial shell (fft_lines.h) and the eikonal backward tile (losses.hip), whose copies once guarded
promises of equal bits.  Text checks only: no GPU, no build."""
import os

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "bubbleformer_amd", "csrc")

LANE_OPS = (
    "void wsync(", "void drain_and_sync(", "void lds_barrier(", "void drain_vm(", "void wait_vm(", "void wait_vm_n(", "void wait_vm_wide(",
    "void glds16(", "void glds16_off(", "void glds16_s(", "unsigned lds_addr(", "void gload4(", "void gload8(", "void gload16(",
    "float dpp_get(", "float dpp_add(", "float row16_sum(", "float quad_sum(", "float quad_max(", "float lane_xor_add(", "float rg8_sum(",
    "s16x4 tr4(", "bf16x8 cat(", "short bfbits(", "float bf_bits_f(", "int t5_bucket(",
    "short s16x8;", "s16x4* lds_s16x4;", "typedef unsigned u32x2 ",
)
BF_COMMON = ("float gelu_erff(", "float dgelu_erff(", "T wave_sum(T v)", "double block_reduce(double v, double* red)")
FFT_LINES = (
    "C* fft_lines(C* x, C* y, const C* tw, const Plan& plan, int lines, int ls)", "void stage(const C* x, C* y, const C* tw, int N, int Ns, int lines, int ls)",
    "void stage_generic(const C* x, C* y, const C* tw, int N, int Ns, int p, int lines, int ls)", "void butterfly(C* v)",
    "int shell_of(long fy, long fx, long H, long W)", "int shell_count(int H, int W)", "Plan make_plan(int n)", "C twiddle(int j, int n)",
    "struct Plan {",
)
OLD_NAMES = ("wave_sync(", "t5b(", "t5_bucket_long(", "tr4g(", "cat8(", "row16_total(", "wave_sum_d(", "gelu_x(", "gelu_e(", "f_bf_bits(",
             "lds_s16x4_ptr", "lds_ptr)", "slp_block_sum(", "wlp_block_sum(")


def _texts():
    return {f: open(os.path.join(CSRC, f)).read() for f in sorted(os.listdir(CSRC)) if f.endswith((".h", ".hip"))}


def test_shared_primitives_are_defined_once():
    texts = _texts()
    for home, sigs in (("lane_ops.h", LANE_OPS), ("bf_common.h", BF_COMMON), ("fft_lines.h", FFT_LINES)):
        for sig in sigs:
            assert {f: t.count(sig) for f, t in texts.items() if sig in t} == {home: 1}, sig


def test_old_helper_names_are_gone():
    texts = _texts()
    for name in OLD_NAMES:
        assert [f for f, t in texts.items() if name in t] == [], name


def test_lane_ops_is_flat_device_code_reached_by_every_user():
    """The header holds device functions and typedefs only (no host state), and a file that calls a helper includes the header itself
    or through gemm_common.h."""
    import re
    texts = _texts()
    h = texts["lane_ops.h"]
    assert '#include "bf_common.h"' in h and '#include "lane_ops.h"' in texts["gemm_common.h"]
    assert not re.search(r"^\s*(static|extern|struct|class|namespace|#define)\b", h, flags=re.M)
    calls = re.compile(r"\b(?:%s)\s*[(<]" % "|".join(s.split("(")[0].split()[-1] for s in LANE_OPS if s.endswith("(")))
    for f, t in texts.items():
        if f.endswith(".hip") and calls.search(t):
            assert '#include "lane_ops.h"' in t or '#include "gemm_common.h"' in t, f


def test_eikonal_backward_tile_is_written_once():
    """eikonal_loss's backward and the interface criterion's penalty gather through one tile body in losses.hip."""
    assert _texts()["losses.hip"].count("eik_weight(j, y, H)") == 1


def test_fft_lines_is_reached_by_every_user():
    import re
    for f, t in _texts().items():
        if f.endswith(".hip") and re.search(r"\bfft_lines\s*\(", t):
            assert '#include "fft_lines.h"' in t, f
