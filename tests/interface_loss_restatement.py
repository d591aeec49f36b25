"""Plain-PyTorch restatement of the interface-weighted criterion (bubbleformer_amd.utils.losses.InterfaceLpLoss) for the parity tests,
written from the maths, in whatever dtype / device the inputs are in.  pred, y are (B, T, C, H, W) in the dataset's normalised units,
stored = (x - diff) / div, `s` the channel of the signed distance:

    phi_t  = y[:, :, s] * div + diff
    w      = 1 + gain * max(0, 1 - |phi_t| / band)                    one map for the C fields of a frame, from the target alone
    rho    = sqrt(sum_hw w (pred - y)^2 / sum_hw w y^2)               per (b, t, c)
    L      = sum_c a_c * mean_{b,t} rho + eikonal * eikonal_loss(pred[:, :, s] * div + diff)

The Eikonal residual is oracle.filmavit_ref.eikonal_loss (spacing 1/32; another spacing rescales the field, the stencil being linear).
`mutant` names one deliberate mistake; the CPU tests require each to move the result by more than the GPU tests' tolerance."""
import torch

from oracle.filmavit_ref import eikonal_loss

DX = 1.0 / 32
MUTANTS = ("weight_from_pred", "unweighted_denominator", "minus_diff", "band_in_cells", "field_weight_inside_root", "no_chain_factor")


def hat(phi, band, gain):
    """1 + gain * max(0, 1 - |phi| / band)"""
    return 1 + gain * (1 - phi.abs() / band).clamp(min=0)


def weight(y, s, band, gain, diff=0.0, div=1.0):
    """(B, T, H, W): the pixel weight of every frame"""
    return hat(y[:, :, s] * div + diff, band, gain) if gain > 0 else torch.ones_like(y[:, :, s])


def row_ratios(pred, y, w):
    """(B, T, C): sqrt(sum w (pred - y)^2 / sum w y^2) over (H, W)"""
    w = w.unsqueeze(2)
    return ((w * (pred - y) ** 2).sum((-2, -1)) / (w * y ** 2).sum((-2, -1))).sqrt()


def field_terms(pred, y, s, band, gain, diff=0.0, div=1.0, field_weights=None, mutant=None):
    """(C,): a_c * mean_{b,t} rho[b, t, c]"""
    C = pred.shape[2]
    a = torch.ones(C, dtype=pred.dtype, device=pred.device) if field_weights is None else torch.as_tensor(field_weights, dtype=pred.dtype, device=pred.device)
    src = pred if mutant == "weight_from_pred" else y
    w = weight(src, s, band * 32 if mutant == "band_in_cells" else band, gain, -diff if mutant == "minus_diff" else diff, div)
    wu = w.unsqueeze(2)
    den = (y ** 2).sum((-2, -1)) if mutant == "unweighted_denominator" else (wu * y ** 2).sum((-2, -1))
    q = (wu * (pred - y) ** 2).sum((-2, -1)) / den
    if mutant == "field_weight_inside_root":
        return (a * q).sqrt().mean((0, 1))
    return a * q.sqrt().mean((0, 1))


def eikonal_term(pred, s, diff=0.0, div=1.0, eikonal=0.0, dx=DX, mutant=None):
    """eikonal * mean (|grad phi_p| - 1)^2 at spacing dx, phi_p = pred[:, :, s] * div + diff"""
    ch = pred[:, :, s]
    phi = ch * div + diff
    if mutant == "no_chain_factor":          # the value of the right expression, the gradient of phi_p taken for the gradient of the channel
        phi = ch + (phi - ch).detach()
    return eikonal * eikonal_loss(phi * (DX / dx))


def loss(pred, y, s, band, gain, diff=0.0, div=1.0, field_weights=None, eikonal=0.0, dx=DX, mutant=None):
    out = field_terms(pred, y, s, band, gain, diff, div, field_weights, mutant).sum()
    if eikonal > 0:
        out = out + eikonal_term(pred, s, diff, div, eikonal, dx, mutant)
    return out


def closed_form_gradient(pred, y, s, band, gain, diff=0.0, div=1.0, field_weights=None, g=1.0):
    """d(g * L_data) / d pred = g * a_c / (B T) * w * (pred - y) / sqrt(S_e S_y)"""
    B, T, C = pred.shape[:3]
    a = torch.ones(C, dtype=pred.dtype, device=pred.device) if field_weights is None else torch.as_tensor(field_weights, dtype=pred.dtype, device=pred.device)
    w = weight(y, s, band, gain, diff, div).unsqueeze(2)
    se, sy = (w * (pred - y) ** 2).sum((-2, -1), keepdim=True), (w * y ** 2).sum((-2, -1), keepdim=True)
    return g * a.view(1, 1, C, 1, 1) / (B * T) * w * (pred - y) / (se * sy).sqrt()


def sdf_fields(shape, seed):
    """Seeded signed-distance-like fields (..., H, W) in the reference's units (grid spacing 1/32), fp64 on the CPU: distance to a circle of
    radius [0.25, 0.75] * min(H, W) / 2 cells around a point of the frame, plus a gentle wave."""
    g = torch.Generator().manual_seed(seed)
    H, W = shape[-2:]
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing="ij")
    lead = shape[:-2]
    cy = torch.rand(lead, generator=g, dtype=torch.float64)[..., None, None] * H
    cx = torch.rand(lead, generator=g, dtype=torch.float64)[..., None, None] * W
    r = (0.25 + 0.5 * torch.rand(lead, generator=g, dtype=torch.float64))[..., None, None] * min(H, W) / 2
    return (torch.sqrt((yy - cy) ** 2 + (xx - cx) ** 2) - r) / 32 + 0.01 * torch.sin(0.3 * yy + cx) * torch.cos(0.2 * xx + cy)


def make_inputs(shape, s, band, diff, div, field_seed=2, noise_seed=1):
    """(pred, y) fp32 on the CPU for a clip shape (B, T, C, H, W): channel s of y is (phi - diff) / div of sdf_fields, the others
    1.5 * randn + 0.25; pred = y + 0.1 * randn * (1 + 2 k), k the hat of height 1 around the interface, so the error is larger inside the band."""
    B, T, C, H, W = shape
    g = torch.Generator().manual_seed(noise_seed)
    phi = sdf_fields((B, T, H, W), field_seed)
    y = torch.randn(shape, generator=g, dtype=torch.float64) * 1.5 + 0.25
    y[:, :, s] = (phi - diff) / div
    y = y.float()
    k = (1 - (y[:, :, s].double() * div + diff).abs() / band).clamp(min=0).unsqueeze(2)
    pred = (y.double() + 0.1 * torch.randn(shape, generator=g, dtype=torch.float64) * (1 + 2 * k)).float()
    return pred, y


def in_band_share(y, s, band, diff, div):
    """(B, T): the share of every frame's cells with |phi_t| < band"""
    return ((y[:, :, s].double() * div + diff).abs() < band).double().mean((-2, -1))
