"""Physics metrics of a rollout, on the device (reference: bubbleformer/utils/losses.py:5-15, bubbleformer/utils/heatflux.py)."""
import ctypes as C
import dataclasses
import math
from typing import Optional, Sequence, Union

import torch

from .. import _lib as L
from ..ops import _p, _require_gpu, _stream


def eikonal_loss(phi: torch.Tensor) -> torch.Tensor:
    """phi = SDF tensor (..., H, W): mean over all elements of (|grad phi| - 1)^2 with dx = 1/32 (utils/losses.py:5-15)."""
    _require_gpu(phi)
    phi = phi.contiguous().float()
    H, W = phi.shape[-2:]
    frames = phi.numel() // (H * W)
    acc = torch.zeros(1, dtype=torch.float64, device=phi.device)
    L.check(L.lib().bf_eikonal_sum(_p(phi), frames, H, W, 1.0 / 32, _p(acc), _stream()), "bf_eikonal_sum")
    return (acc / phi.numel()).float().squeeze(0)


def eikonal_l1_per_frame(phi: torch.Tensor) -> torch.Tensor:
    """phi (T, H, W) SDF frames -> (T,) scores of the rollout notebook (`get_eikonal_loss`, scripts/inference_autoregressive.ipynb):
    mean | |grad phi| - 1 | per frame, central differences at dx = 1/32 with replicate-padded borders."""
    _require_gpu(phi)
    if phi.dim() != 3:
        raise ValueError("eikonal_l1_per_frame expects (T, H, W)")
    phi = phi.contiguous().float()
    T, H, W = phi.shape
    out = torch.empty(T, dtype=torch.float32, device=phi.device)
    L.check(L.lib().bf_eikonal_l1_frames(_p(phi), T, H, W, 1.0 / 32, _p(out), _stream()), "bf_eikonal_l1_frames")
    return out


def heatflux(dfun: torch.Tensor, temp: torch.Tensor, heater_temp: float):
    """FC-72 heater heat flux (utils/heatflux.py:3-38): dfun, temp (T, 512, 512) device tensors -> (mean, max) over frames of the
    bottom-row flux.  The reference hard-codes the 16 x 16 domain at dx = 1/32 (512 x 512 cells); so does this."""
    _require_gpu(dfun)
    if tuple(dfun.shape[1:]) != (512, 512) or dfun.shape != temp.shape:
        raise ValueError("heatflux expects (T, 512, 512) fields (utils/heatflux.py:21-33)")
    dfun, temp = dfun.contiguous().float(), temp.contiguous().float()
    T = dfun.shape[0]
    flux = torch.empty(T, dtype=torch.float32, device=dfun.device)
    L.check(L.lib().bf_heatflux_rows(_p(dfun), _p(temp), T, 512 * 512, 512, -8.0, 1.0 / 32, float(heater_temp), 0.0007, _p(flux), _stream()),
            "bf_heatflux_rows")
    return flux.mean(), flux.max()


@dataclasses.dataclass(frozen=True)
class HeaterSpec:
    """The heater of a pool-boiling study, for the heat flux of utils/heatflux.py.  The defaults are the reference's FC-72 constants
    (heatflux.py:17-35); ``heater_temp`` is one float, or one float per file of the dataset.  The domain is symmetric about x = 0, as the
    reference assumes (x in [-8, 8) at dx = 1/32: 512 columns), so a downsampled or coarser dataset needs a spec with its own ``dx``."""
    heater_temp: Union[float, Sequence[float]]
    temperature_field: str = "temperature"
    sdf_field: str = "dfun"
    x_min: float = -8.0
    dx: float = 1.0 / 32
    lc: float = 0.0007
    conductivity: float = 0.054

    def check_width(self, W: int) -> None:
        """A frame of W columns is accepted when x_min + W * dx = -x_min to 1e-9 relative (the slack is for a dx that is no binary fraction)."""
        x_max = self.x_min + int(W) * self.dx
        if not (self.dx > 0 and self.lc > 0 and abs(x_max + self.x_min) <= 1e-9 * abs(self.x_min)):
            raise ValueError(f"a frame of {W} columns at dx = {self.dx} ends at x = {x_max}, the symmetric domain of utils/heatflux.py at "
                             f"{-self.x_min}: give the HeaterSpec the dataset's own dx")

    def temperatures(self, files: Sequence[int], num_files: int) -> list:
        """heater_temp of every trajectory, from the file each comes from."""
        if isinstance(self.heater_temp, (int, float)):
            return [float(self.heater_temp)] * len(files)
        temps = [float(v) for v in self.heater_temp]
        if len(temps) != int(num_files):
            raise ValueError(f"heater_temp has {len(temps)} entries, the dataset {num_files} files: give one float, or one per file")
        return [temps[int(f)] for f in files]

    def channels(self, fields: Sequence[str]):
        """(signed-distance channel, temperature channel) among the output fields."""
        fields = list(fields)
        for name in (self.sdf_field, self.temperature_field):
            if name not in fields:
                raise ValueError(f"the heat flux needs the field {name!r} among the output fields {fields}")
        return fields.index(self.sdf_field), fields.index(self.temperature_field)


def heatflux_series(dfun: torch.Tensor, temp: torch.Tensor, heater_temp: float, spec: Optional[HeaterSpec] = None) -> torch.Tensor:
    """dfun, temp (T, H, W) device tensors in physical units -> (T,) fp32: the bottom-row heat flux of every frame (the `hfluxes` of
    utils/heatflux.py:36, which ``heatflux`` reduces to mean and max), for any width the spec accepts."""
    _require_gpu(dfun)
    spec = spec if spec is not None else HeaterSpec(heater_temp)
    if dfun.dim() != 3 or dfun.shape != temp.shape:
        raise ValueError(f"heatflux_series expects two (T, H, W) fields of one shape, got {tuple(dfun.shape)} and {tuple(temp.shape)}")
    T, H, W = dfun.shape
    spec.check_width(W)
    dfun, temp = dfun.contiguous().float(), temp.contiguous().float()
    flux = torch.empty(T, dtype=torch.float32, device=dfun.device)
    # bf_heatflux_rows carries the reference's conductivity 0.054 in its coefficient 0.054 / (dx * lc): another conductivity scales lc
    # (a factor of exactly 1 at the default, so the default spec has the bits ``heatflux`` reduces)
    lc = spec.lc * (0.054 / spec.conductivity)
    L.check(L.lib().bf_heatflux_rows(_p(dfun), _p(temp), T, H * W, W, float(spec.x_min), float(spec.dx), float(heater_temp), float(lc), _p(flux),
                                     _stream()), "bf_heatflux_rows")
    return flux


def kde_kl_divergence(sim: torch.Tensor, model: torch.Tensor, points: int = 1000, eps: float = 1e-10, return_pdfs: bool = False):
    """KL(sim || model) of the Gaussian kernel density estimates of two sample sets, as examples/data_visualization.ipynb cell 4 computes it
    (scipy's gaussian_kde with Scott's bandwidth, a ``points``-point grid over both sets, Simpson's rule), on the device in fp64 without a
    points x n intermediate.  sim (n,) / model (m,), or batched (R, n) / (R, m), fp32 or fp64 -> a 0-d or (R,) fp64 tensor; with
    ``return_pdfs`` also (x, pdf_sim, pdf_model), each (points,) or (R, points).  One deviation from the notebook: where the simulated
    density is exactly 0 the integrand is 0 (its limit) instead of numpy's NaN.  A set of zero variance gives NaN.  Never synchronises."""
    from .. import ops
    _require_gpu(sim)
    if sim.dim() not in (1, 2) or sim.dim() != model.dim() or (sim.dim() == 2 and sim.shape[0] != model.shape[0]):
        raise ValueError(f"kde_kl_divergence expects (n,) and (m,), or (R, n) and (R, m); got {tuple(sim.shape)} and {tuple(model.shape)}")
    single = sim.dim() == 1
    p = sim.reshape(1 if single else sim.shape[0], -1).to(torch.float64).contiguous()
    q = model.reshape(p.shape[0], -1).to(torch.float64).contiguous()
    if p.shape[1] < 2 or q.shape[1] < 2 or int(points) < 3:
        raise ValueError(f"kde_kl_divergence needs at least 2 samples per set and 3 grid points (got {p.shape[1]}, {q.shape[1]}, {points})")
    R = p.shape[0]
    new = lambda *shape: torch.empty(shape, dtype=torch.float64, device=p.device)
    kl = new(R)
    extra = (new(R, points), new(R, points), new(R, points)) if return_pdfs else (None, None, None)
    ops.kde_kl(p, q, int(points), float(eps), ops.kde_kl_workspace(R, p.shape[1], q.shape[1], int(points), p.device), kl, *extra)
    if not return_pdfs:
        return kl[0] if single else kl
    return (kl[0],) + tuple(t[0] for t in extra) if single else (kl,) + extra


@dataclasses.dataclass(frozen=True, eq=False)
class BubbleSpec:
    """The bubble census of a rollout (``evaluate_rollouts(..., bubbles=BubbleSpec())``): which output field is the signed distance, how cells
    connect (4: edges, 8: edges and corners), how many per-bubble records a frame keeps, and the cell size for the equivalent diameters.  With
    ``track`` the bubbles are also followed from frame to frame (``bubble_tracks``): the report gains the link, event and departure rows.  With
    ``match`` the predicted bubbles of every frame are matched to the simulated ones (``bubble_match``; ``min_iou`` is its IoU bound): the report
    gains the match rows and the detection scores."""
    sdf_field: str = "dfun"
    connectivity: int = 4
    max_bubbles: int = 256
    dx: float = 1.0 / 32
    track: bool = False
    # constructor arguments behind `track`, by position or by name, and attributes of the instance; dataclasses.fields() ends at `track` as before
    match: dataclasses.InitVar[bool] = False
    min_iou: dataclasses.InitVar[float] = 0.0

    def __post_init__(self, match, min_iou):
        _check_census_arguments(self.connectivity, self.max_bubbles)
        if not isinstance(self.track, bool):
            raise ValueError(f"track must be True or False, got {self.track!r}")
        if not isinstance(match, bool):
            raise ValueError(f"match must be True or False, got {match!r}")
        _check_min_iou(min_iou)
        if (self.track or match) and int(self.max_bubbles) > MAX_TRACKED_BUBBLES:
            raise ValueError(f"tracking and matching keep at most {MAX_TRACKED_BUBBLES} records per frame, got max_bubbles = {self.max_bubbles}")
        if not self.dx > 0:
            raise ValueError(f"dx must be positive, got {self.dx}")
        object.__setattr__(self, "match", match)
        object.__setattr__(self, "min_iou", float(min_iou))

    def _key(self):
        return dataclasses.astuple(self) + (self.match, self.min_iou)

    def __eq__(self, other):
        return self._key() == other._key() if isinstance(other, BubbleSpec) else NotImplemented

    def __hash__(self):
        return hash(self._key())

    def __repr__(self):
        return "BubbleSpec(" + ", ".join(f"{f.name}={getattr(self, f.name)!r}" for f in dataclasses.fields(self)) + f", match={self.match!r}, min_iou={self.min_iou!r})"

    def channel(self, fields: Sequence[str]) -> int:
        """The signed-distance channel among the output fields."""
        fields = list(fields)
        if self.sdf_field not in fields:
            raise ValueError(f"the bubble census needs the field {self.sdf_field!r} among the output fields {fields}")
        return fields.index(self.sdf_field)


MAX_TRACKED_BUBBLES = 1 << 15          # bf_bubble_links' limit: an overlap table of max_bubbles^2 int32 indices


def _check_min_iou(min_iou) -> None:
    if isinstance(min_iou, bool) or not isinstance(min_iou, (int, float)) or not 0.0 <= float(min_iou) <= 1.0:        # a NaN fails both comparisons
        raise ValueError(f"min_iou must be a number in [0, 1], got {min_iou!r}")


def _check_census_arguments(connectivity, max_bubbles) -> None:
    if connectivity not in (4, 8):
        raise ValueError(f"connectivity must be 4 or 8, got {connectivity!r}")
    if int(max_bubbles) != max_bubbles or int(max_bubbles) < 1:
        raise ValueError(f"max_bubbles must be an integer of at least 1, got {max_bubbles!r}")


def equivalent_diameter(area: torch.Tensor, dx: float = 1.0 / 32) -> torch.Tensor:
    """The diameter of the disc of a bubble's area, 2 * sqrt(area * dx^2 / pi) in fp32; 0 where the area is 0 (an unused slot)."""
    return 2.0 * torch.sqrt(area.to(torch.float32) * (float(dx) * float(dx) / math.pi))


@dataclasses.dataclass
class BubbleCensus:
    """What ``bubble_census`` returns; every tensor is on the device and keeps phi's leading dims.  The bubbles of a frame are numbered in raster
    order of their first cell (scipy.ndimage.label's numbering); slot k of the records is bubble k + 1, slots behind the last bubble are 0."""
    count: torch.Tensor                             # (...)                 int32: components of the frame, also above max_bubbles
    vapour_cells: torch.Tensor                      # (...)                 int32: cells with phi > 0
    attached: torch.Tensor                          # (...)                 int32: components with a cell in row 0 (the heater row)
    area: torch.Tensor                              # (..., max_bubbles)    int32 cells
    centroid: torch.Tensor                          # (..., max_bubbles, 2) fp32 (y, x) in cells
    on_heater: torch.Tensor                         # (..., max_bubbles)    bool
    shape: tuple                                    # (H, W)
    labels: Optional[torch.Tensor] = None           # (..., H, W)           int32, 0 = liquid, if asked for

    def vapour_fraction(self) -> torch.Tensor:
        """vapour_cells / (H * W): the quotient in fp64, rounded once to fp32."""
        return (self.vapour_cells.to(torch.float64) / float(self.shape[0] * self.shape[1])).to(torch.float32)

    def equivalent_diameter(self, dx: float = 1.0 / 32) -> torch.Tensor:
        """(..., max_bubbles) fp32: 2 * sqrt(area * dx^2 / pi) of every record, 0 in unused slots."""
        return equivalent_diameter(self.area, dx)


def bubble_census(phi: torch.Tensor, *, connectivity: int = 4, max_bubbles: int = 256, return_labels: bool = False) -> BubbleCensus:
    """The bubbles of every frame of phi (..., H, W), a signed-distance field in physical units on the device.  Vapour is phi > 0: an exact
    zero and a NaN count as liquid.  A bubble is a connected component of vapour cells under ``connectivity`` 4 (edges) or 8 (edges and
    corners); row 0 is the heater row.  One launch, a workgroup per frame (``ops.bubble_census``); never synchronises; the same bits on every
    call, and for a frame alone or in a batch.  A frame of more than 2^24 cells raises ``BubbleformerHipError`` before any launch."""
    _check_census_arguments(connectivity, max_bubbles)
    if phi.dim() < 2:
        raise ValueError(f"bubble_census expects (..., H, W), got {tuple(phi.shape)}")
    from .. import ops
    _require_gpu(phi)
    lead, (H, W) = tuple(phi.shape[:-2]), phi.shape[-2:]
    mb = int(max_bubbles)
    flat = phi.reshape(-1, H, W).contiguous().float()
    F = flat.shape[0]
    if F < 1 or H < 1 or W < 1:
        raise ValueError(f"bubble_census needs at least one frame of at least one cell, got {tuple(phi.shape)}")
    ws = ops.bubble_census_workspace(F, H, W, mb, flat.device)
    new = lambda dtype, *shape: torch.empty(shape, dtype=dtype, device=flat.device)
    count, cells, attached, area = new(torch.int32, F), new(torch.int32, F), new(torch.int32, F), new(torch.int32, F, mb)
    centroid, on_heater = new(torch.float32, F, mb, 2), new(torch.bool, F, mb)
    labels = new(torch.int32, F, H, W) if return_labels else None
    ops.bubble_census(flat, int(connectivity), mb, ws, count, cells, attached, area, centroid, on_heater, labels)
    return BubbleCensus(count.reshape(lead), cells.reshape(lead), attached.reshape(lead), area.reshape(lead + (mb,)), centroid.reshape(lead + (mb, 2)),
                        on_heater.reshape(lead + (mb,)), (int(H), int(W)), labels.reshape(lead + (int(H), int(W))) if labels is not None else None)


def _check_redistance_arguments(dx, band, max_rounds) -> None:
    if not dx > 0:
        raise ValueError(f"dx must be positive, got {dx}")
    if band is not None and not band > 0:
        raise ValueError(f"band must be None or positive, got {band}")
    if max_rounds is not None and (int(max_rounds) != max_rounds or int(max_rounds) < 1):
        raise ValueError(f"max_rounds must be None or an integer of at least 1, got {max_rounds!r}")


@dataclasses.dataclass(frozen=True)
class RedistanceSpec:
    """Redistancing of the predicted signed-distance field during a rollout (``evaluate_rollouts_redistanced(..., RedistanceSpec())``): the cell
    size, the distance cap (None: none), the pass limit (None: H + W), and ``every``: the correction runs on the steps s with (s + 1) % every == 0.
    The scheme is first order and moves the interpolated zero crossings by a few hundredths of a cell per application, so on a long rollout a
    larger ``every`` keeps the interface from creeping."""
    dx: float = 1.0 / 32
    band: Optional[float] = None
    max_rounds: Optional[int] = None
    every: int = 1
    sdf_field: str = "dfun"

    def __post_init__(self):
        _check_redistance_arguments(self.dx, self.band, self.max_rounds)
        if int(self.every) != self.every or int(self.every) < 1:
            raise ValueError(f"every must be an integer of at least 1, got {self.every!r}")

    def channel(self, fields: Sequence[str]) -> int:
        """The signed-distance channel among the output fields."""
        fields = list(fields)
        if self.sdf_field not in fields:
            raise ValueError(f"redistancing needs the field {self.sdf_field!r} among the output fields {fields}")
        return fields.index(self.sdf_field)


def redistance(phi: torch.Tensor, dx: float = 1.0 / 32, band: Optional[float] = None, max_rounds: Optional[int] = None,
               out: Optional[torch.Tensor] = None, return_status: bool = False):
    """The signed distance to the zero level set of every frame of phi (..., H, W), an fp32 field in physical units on the device, by
    first-order redistancing at spacing ``dx`` (``ops.redistance``): interface cells take the distance to the linearly
    interpolated crossings and are frozen, the others the Godunov upwind solution of |grad d| = 1, capped at ``band`` if given.  The signs and
    the interface cells are those of phi exactly.  ``out`` (like phi, contiguous; may be phi) receives the result.  With ``return_status``
    -> (result, rounds, change_rms), both of phi's leading dims: rounds int32 >= 1 passes run, 0 a one-sign frame (unchanged), -1 a non-finite
    frame (unchanged), -2 ``max_rounds`` (default H + W) ran out; change_rms fp32 the root mean square change.  One launch, a workgroup per
    frame; never synchronises; the same bits on every call, and for a frame alone or in a batch."""
    _check_redistance_arguments(dx, band, max_rounds)
    if phi.dim() < 2:
        raise ValueError(f"redistance expects (..., H, W), got {tuple(phi.shape)}")
    if phi.numel() < 1:                               # before any reshape: a zero-sized axis has no frame to name
        raise ValueError(f"redistance needs at least one frame of at least one cell, got {tuple(phi.shape)}")
    from .. import ops
    _require_gpu(phi)
    if phi.dtype != torch.float32:
        raise L.BubbleformerHipError(f"redistance: phi must be fp32, got {phi.dtype}")
    lead, (H, W) = tuple(phi.shape[:-2]), (int(phi.shape[-2]), int(phi.shape[-1]))
    flat = phi.reshape(-1, H, W).contiguous()
    F = flat.shape[0]
    if out is None:
        result = torch.empty_like(flat)
    else:
        if out.shape != phi.shape or out.dtype != torch.float32 or not out.is_contiguous() or out.device != phi.device:
            raise L.BubbleformerHipError(f"redistance: out must be a contiguous fp32 tensor of shape {tuple(phi.shape)} on {phi.device}")
        result = out.view(-1, H, W)
    rounds = torch.empty(F, dtype=torch.int32, device=flat.device) if return_status else None
    change = torch.empty(F, dtype=torch.float32, device=flat.device) if return_status else None
    ops.redistance(flat, float(dx), band, max_rounds, ops.redistance_workspace(F, H, W, flat.device), result, rounds, change)
    result = out if out is not None else result.reshape(phi.shape)
    return (result, rounds.reshape(lead), change.reshape(lead)) if return_status else result


def departure_diameters(departure_area: torch.Tensor, dx: float = 1.0 / 32) -> torch.Tensor:
    """The equivalent diameters of the bubbles that leave the heater, a 1-D fp32 device tensor in row order, from ``departure_area`` rows (area at
    the departing bubble's slot, 0 elsewhere, -1 in an invalid pair).  SYNCHRONISES: dropping the empty slots makes the host wait for their number."""
    return equivalent_diameter(departure_area[departure_area > 0], dx)


def departure_frequency(events: torch.Tensor) -> torch.Tensor:
    """events (..., pairs, 5) -> (...) fp64: departures per frame pair, over the valid pairs (NaN without one).  On the device; never synchronises."""
    departures = events[..., 4]
    valid = departures >= 0
    return departures.clamp(min=0).sum(-1).to(torch.float64) / valid.sum(-1).to(torch.float64)


@dataclasses.dataclass
class BubbleTracks:
    """What ``bubble_tracks`` returns; every tensor is int32 on the device and keeps phi's leading dims.  Pair t is frames t and t + 1; slot k of a
    row is bubble k + 1 of the pair's earlier (successor, n_successors, departure_area) or later (predecessor, n_predecessors) frame; 0 means none."""
    census: BubbleCensus                            # of every frame, label images included
    successor: torch.Tensor                         # (..., T-1, max_bubbles)  the later frame's bubble that shares most cells, ties to the smallest
    n_successors: torch.Tensor                      # (..., T-1, max_bubbles)  how many share a cell
    predecessor: torch.Tensor                       # (..., T-1, max_bubbles)
    n_predecessors: torch.Tensor                    # (..., T-1, max_bubbles)
    departure_area: torch.Tensor                    # (..., T-1, max_bubbles)  cells of a bubble that leaves the heater row in this pair, else 0
    events: torch.Tensor                            # (..., T-1, 5)            births, deaths, merges, splits, departures
    track_id: torch.Tensor                          # (..., T, max_bubbles)    1, 2, ... per sequence by first appearance, 0 in unused slots
    n_tracks: torch.Tensor                          # (...)

    def departure_diameters(self, dx: float = 1.0 / 32) -> torch.Tensor:
        """The equivalent diameters of all departing bubbles, a 1-D fp32 device tensor in pair order.  SYNCHRONISES (it compacts)."""
        return departure_diameters(self.departure_area, dx)

    def lifetimes(self) -> torch.Tensor:
        """Frames every track lives, a 1-D int64 device tensor: the tracks of the first sequence in id order, then the next one's.  SYNCHRONISES
        (it compacts).  A track cut by the first or last frame counts the frames it was seen."""
        mb = self.track_id.shape[-1]
        T = self.track_id.shape[-2]
        ids = self.track_id.reshape(-1, T * mb).to(torch.int64)
        seen = torch.zeros(ids.shape[0], T * mb + 1, dtype=torch.int64, device=ids.device).scatter_add_(1, ids, torch.ones_like(ids))[:, 1:]
        return seen[seen > 0]

    def departure_frequency(self) -> torch.Tensor:
        """(...) fp64: departures per frame pair of every sequence.  On the device; never synchronises."""
        return departure_frequency(self.events)


def bubble_tracks(phi: torch.Tensor, *, connectivity: int = 4, max_bubbles: int = 256) -> BubbleTracks:
    """The bubbles of phi (..., T, H, W), a signed-distance field in physical units on the device, followed along axis -3: the census of every
    frame with its label images (``bubble_census``), the links of every consecutive pair and their events (``ops.bubble_links``, a workgroup per
    pair) and the track ids (``ops.bubble_track_ids``, a workgroup per sequence).  Three launches (one for T = 1: its pair tensors are empty);
    never synchronises; the same bits on every call, and for a sequence alone or in a batch."""
    _check_census_arguments(connectivity, max_bubbles)
    if phi.dim() < 3:
        raise ValueError(f"bubble_tracks expects (..., T, H, W), got {tuple(phi.shape)}")
    if int(max_bubbles) > MAX_TRACKED_BUBBLES:
        raise ValueError(f"tracking keeps at most {MAX_TRACKED_BUBBLES} records per frame, got max_bubbles = {max_bubbles}")
    from .. import ops
    census = bubble_census(phi, connectivity=connectivity, max_bubbles=max_bubbles, return_labels=True)
    lead, (T, H, W), mb = tuple(phi.shape[:-3]), phi.shape[-3:], int(max_bubbles)
    N = census.count.numel() // T
    new = lambda *shape: torch.empty(shape, dtype=torch.int32, device=phi.device)
    rows = {k: new(*shape) for k, shape in ops._link_rows((N, T - 1), mb).items()}
    if T > 1:
        ops.bubble_links(census.labels.reshape(N, T, H, W), census.count.reshape(N, T), census.attached.reshape(N, T), census.area.reshape(N, T, mb),
                         ops.bubble_links_workspace(N * (T - 1), mb, phi.device), **rows)
    track_id, n_tracks = new(N, T, mb), new(N)
    ops.bubble_track_ids(census.count.reshape(N, T), rows["successor"], rows["predecessor"], track_id, n_tracks)
    return BubbleTracks(census, **{k: v.reshape(lead + v.shape[1:]) for k, v in rows.items()}, track_id=track_id.reshape(lead + (T, mb)),
                        n_tracks=n_tracks.reshape(lead))


def _quotient(num: torch.Tensor, den: torch.Tensor) -> torch.Tensor:
    """num / den in fp64, rounded once to fp32; NaN where den is 0."""
    den = den.to(torch.float64)
    return (num.to(torch.float64) / torch.where(den == 0, torch.full_like(den, float("nan")), den)).to(torch.float32)


def detection_scores(counts: torch.Tensor, attached: bool = False):
    """counts (..., 6) int32 as ``bubble_match`` leaves them -> (precision, recall, csi), each (...) fp32: hits / (hits + false alarms), hits /
    (hits + misses), hits / (hits + misses + false alarms), of all bubbles or with ``attached`` of those on the heater.  Every quotient in fp64,
    rounded once; NaN where the denominator is 0 and in an invalid pair (-1).  On the device; never synchronises."""
    hits, misses, alarms = (counts[..., (3 if attached else 0) + q].to(torch.float64) for q in range(3))
    bad = torch.full_like(hits, float("nan"))
    hits = torch.where(hits < 0, bad, hits)
    return _quotient(hits, hits + alarms), _quotient(hits, hits + misses), _quotient(hits, hits + misses + alarms)


def mask_iou(mask: torch.Tensor) -> torch.Tensor:
    """mask (..., 2) int32 (cells vapour on both sides, on either) -> (...) fp32 IoU of the whole vapour mask: the quotient in fp64, rounded once;
    NaN where neither side has vapour and in an invalid pair (-1)."""
    both = mask[..., 0].to(torch.float64)
    return _quotient(torch.where(both < 0, torch.full_like(both, float("nan")), both), mask[..., 1])


def matched_iou(overlap: torch.Tensor, match_pred: torch.Tensor, area_pred: torch.Tensor, area_target: torch.Tensor) -> torch.Tensor:
    """(..., max_bubbles) fp32 per predicted slot: overlap / (area_pred[i] + area_target[match] - overlap) of a matched pair, the quotient in
    fp64, rounded once; NaN in unmatched and unused slots and in an invalid pair."""
    matched = match_pred > 0
    partner = torch.gather(area_target, -1, (match_pred.to(torch.int64) - 1).clamp(min=0))
    union = torch.where(matched, area_pred + partner - overlap, torch.zeros_like(overlap))
    return _quotient(overlap, union)


def centroid_error(displacement: torch.Tensor, match_pred: torch.Tensor, dx: float = 1.0) -> torch.Tensor:
    """(...) fp32: the mean centroid displacement of a frame's matched pairs times ``dx`` (the sum and the quotient in fp64, rounded once); NaN
    where a frame has no matched pair."""
    matched = match_pred > 0
    total = torch.where(matched, displacement.to(torch.float64), torch.zeros((), dtype=torch.float64, device=displacement.device)).sum(-1)
    return _quotient(total * float(dx), matched.sum(-1))


@dataclasses.dataclass
class BubbleMatch:
    """What ``bubble_match`` returns; every tensor is on the device and keeps the fields' leading dims.  Slot k of match_pred, overlap and
    displacement is predicted bubble k + 1, slot k of match_target simulated bubble k + 1; 0 means unmatched or unused."""
    match_pred: torch.Tensor                        # (..., max_bubbles) int32  the matched simulated bubble
    match_target: torch.Tensor                      # (..., max_bubbles) int32  the matched predicted bubble
    overlap: torch.Tensor                           # (..., max_bubbles) int32  cells the matched pair shares
    displacement: torch.Tensor                      # (..., max_bubbles) fp32   distance between the pair's centroids, in cells
    counts: torch.Tensor                            # (..., 6) int32            hits, misses, false alarms; the same three on the heater
    mask: torch.Tensor                              # (..., 2) int32            cells vapour on both sides, on either
    count_pred: torch.Tensor                        # (...) int32               the two censuses' rows
    count_target: torch.Tensor
    attached_pred: torch.Tensor
    attached_target: torch.Tensor
    area_pred: torch.Tensor                         # (..., max_bubbles) int32
    area_target: torch.Tensor

    def iou(self) -> torch.Tensor:
        """(..., max_bubbles) fp32: the IoU of every matched pair at the predicted bubble's slot, NaN elsewhere."""
        return matched_iou(self.overlap, self.match_pred, self.area_pred, self.area_target)

    def precision(self, attached: bool = False) -> torch.Tensor:
        return detection_scores(self.counts, attached)[0]

    def recall(self, attached: bool = False) -> torch.Tensor:
        return detection_scores(self.counts, attached)[1]

    def csi(self, attached: bool = False) -> torch.Tensor:
        """The critical success index hits / (hits + misses + false alarms); as precision and recall NaN where the denominator is 0."""
        return detection_scores(self.counts, attached)[2]

    def mask_iou(self) -> torch.Tensor:
        return mask_iou(self.mask)

    def centroid_error(self, dx: float = 1.0 / 32) -> torch.Tensor:
        """(...) fp32: the mean centroid displacement of every frame's matched pairs, in units of ``dx`` per cell."""
        return centroid_error(self.displacement, self.match_pred, dx)


def bubble_match(phi_pred: torch.Tensor, phi_target: torch.Tensor, *, connectivity: int = 4, max_bubbles: int = 256, min_iou: float = 0.0) -> BubbleMatch:
    """The bubbles of phi_pred matched to those of phi_target, two (..., H, W) signed-distance fields of one shape in physical units on the
    device, frame by frame: a predicted and a simulated bubble are matched when each is the other's largest overlap and
    their IoU is at least ``min_iou``.  Two labelled censuses (``bubble_census``), then one launch, a workgroup per frame pair
    (``ops.bubble_match``); never synchronises; the same bits on every call, and for a pair alone or in a batch."""
    _check_census_arguments(connectivity, max_bubbles)
    _check_min_iou(min_iou)
    if phi_pred.dim() < 2 or phi_pred.shape != phi_target.shape:
        raise ValueError(f"bubble_match expects two (..., H, W) fields of one shape, got {tuple(phi_pred.shape)} and {tuple(phi_target.shape)}")
    if int(max_bubbles) > MAX_TRACKED_BUBBLES:
        raise ValueError(f"matching keeps at most {MAX_TRACKED_BUBBLES} records per frame, got max_bubbles = {max_bubbles}")
    from .. import ops
    sides = [bubble_census(phi, connectivity=connectivity, max_bubbles=max_bubbles, return_labels=True) for phi in (phi_pred, phi_target)]
    lead, (H, W), mb = tuple(phi_pred.shape[:-2]), phi_pred.shape[-2:], int(max_bubbles)
    F = sides[0].count.numel()
    rows = {k: torch.empty((F,) + shape[1:], dtype=dtype, device=phi_pred.device) for k, (shape, dtype) in ops._match_rows((F,), mb).items()}
    ops.bubble_match(*(c.labels.reshape(F, H, W) for c in sides), *(c.count.reshape(F) for c in sides), *(c.attached.reshape(F) for c in sides),
                     *(c.area.reshape(F, mb) for c in sides), float(min_iou), ops.bubble_match_workspace(F, mb, phi_pred.device), rows)
    p, s = sides
    return BubbleMatch(**{k: v.reshape(lead + v.shape[1:]) for k, v in rows.items()}, count_pred=p.count, count_target=s.count,
                       attached_pred=p.attached, attached_target=s.attached, area_pred=p.area, area_target=s.area)


@dataclasses.dataclass(frozen=True)
class ErrorSpec:
    """The error rows of a rollout (``evaluate_rollouts(..., errors=ErrorSpec())``) or of ``field_errors``: how far from a cell the window that
    decides "at the interface" reaches, the shells (lo, hi) that split the low, mid and high band, whether the spectra are taken at all, and
    which output field is the signed distance."""
    interface_radius: int = 1
    bands: tuple = (4, 12)
    spectra: bool = True
    sdf_field: str = "dfun"

    def __post_init__(self):
        if int(self.interface_radius) != self.interface_radius or int(self.interface_radius) < 1:
            raise ValueError(f"interface_radius must be an integer of at least 1, got {self.interface_radius!r}")
        try:
            lo, hi = self.bands
            ok = int(lo) == lo and int(hi) == hi and 0 <= lo <= hi
        except (TypeError, ValueError):
            ok = False
        if not ok:
            raise ValueError(f"bands must be two integers 0 <= lo <= hi, got {self.bands!r}")


def shell_count(H: int, W: int) -> int:
    """The number of shells of an H x W frame's spectrum: isqrt(S * S // 2) + 1 with S = min(H, W)."""
    from ..ops import shell_count as count
    return count(H, W)


@dataclasses.dataclass
class FieldErrors:
    """What ``field_errors`` returns; every tensor is on the device and keeps the leading dims of the prediction.  e = pred - target in fp64."""
    rmse: torch.Tensor                              # (...)     fp32  sqrt(mean e^2)
    max_error: torch.Tensor                         # (...)     fp32  max |e|; NaN if any e is NaN
    boundary_rmse: torch.Tensor                     # (...)     fp32  the root mean square over the outer ring of cells
    interface_rmse: Optional[torch.Tensor]          # (...)     fp32  the same over the interface cells of sdf (NaN where there is none), or None
    interface_cells: Optional[torch.Tensor]         # (...)     int32 their number
    spectral_error: Optional[torch.Tensor]          # (..., 3)  fp32  band-limited RMSE of e: low, mid, high; None without spectra
    spectrum_error: Optional[torch.Tensor]          # (..., K)  fp32  shell power of e
    spectrum_pred: Optional[torch.Tensor]           # (..., K)  fp32  shell power of the prediction
    spectrum_target: Optional[torch.Tensor]         # (..., K)  fp32  shell power of the target

    def spectral_ratio(self) -> torch.Tensor:
        """spectrum_pred / spectrum_target per shell: the blurring curve (below 1 where the prediction lost power).  Never synchronises."""
        if self.spectrum_pred is None:
            raise ValueError("these errors have no spectra: use ErrorSpec(spectra=True)")
        return self.spectrum_pred / self.spectrum_target


def field_errors(pred: torch.Tensor, target: torch.Tensor, sdf: Optional[torch.Tensor] = None, *, spec: ErrorSpec = ErrorSpec()) -> FieldErrors:
    """Where ``pred`` (..., H, W) differs from ``target`` and at which scales, per frame, on the device (``ops.field_errors``).

    Pointwise rows: RMSE, maximum error, RMSE over the outer ring, and -- with ``sdf`` (same shape, physical units: vapour is sdf > 0) -- RMSE
    over the cells whose (2 r + 1)^2 window holds both vapour and liquid, with their number.  Spectra: the power of e, pred and target per
    shell of the unnormalised 2-D DFT divided by (H W)^2, so a field's shells add up to its mean square, and ``spectral_error``, the
    band-limited RMSE sqrt(sum of the error's shell power over the band) for the bands [0, lo), [lo, hi), [hi, K): low^2 + mid^2 + high^2 =
    rmse^2.  This is NOT PDEBench's fRMSE, which is the mean over a band of the per-shell roots.  fp64 arithmetic, one rounding, the same
    bits on every call and for a frame alone or in a batch; never synchronises."""
    if pred.dim() < 2 or pred.shape != target.shape or (sdf is not None and sdf.shape != pred.shape):
        raise ValueError(f"field_errors expects pred, target (and sdf) of one shape (..., H, W), got {tuple(pred.shape)} and {tuple(target.shape)}")
    from .. import ops
    _require_gpu(pred)
    lead, (H, W) = tuple(pred.shape[:-2]), pred.shape[-2:]
    flat = lambda t: t.reshape(-1, H, W).contiguous().float()
    p, y, phi = flat(pred), flat(target), flat(sdf) if sdf is not None else None
    F = p.shape[0]
    if F < 1 or H < 1 or W < 1:
        raise ValueError(f"field_errors needs at least one frame of at least one cell, got {tuple(pred.shape)}")
    K = shell_count(H, W)
    new = lambda dtype, *shape: torch.empty(shape, dtype=dtype, device=p.device)
    rows = {"rmse": new(torch.float32, F), "max_error": new(torch.float32, F), "boundary_rmse": new(torch.float32, F)}
    if phi is not None:
        rows["interface_rmse"], rows["interface_cells"] = new(torch.float32, F), new(torch.int32, F)
    if spec.spectra:
        rows["spectral_error"] = new(torch.float32, F, 3)
        for key in ("spectrum_error", "spectrum_pred", "spectrum_target"):
            rows[key] = new(torch.float32, F, K)
    ops.field_errors(p, y, phi, ops.field_errors_workspace(F, H, W, p.device), int(spec.interface_radius), int(spec.bands[0]), int(spec.bands[1]),
                     spec.spectra, **rows)
    return FieldErrors(**{k: (rows[k].reshape(lead + tuple(rows[k].shape[1:])) if k in rows else None) for k in ops._ERROR_ROWS})


@dataclasses.dataclass(frozen=True)
class FlowSpec:
    """The flow-consistency rows of a rollout (``evaluate_rollouts_flow(..., FlowSpec(dt))``) or of ``flow_consistency``: ``dt``, the time between
    two stored frames in the units of ``dx`` over velocity -- it has NO default: neither the reference nor the dataset carries it, and a wrong one
    would silently scale the transport residual -- the cell size, the half-width of the band around the interface in which the transport residual
    is taken (None: 3 dx), how far from a cell the window that decides "bulk liquid" reaches, and which output fields are the signed distance and
    the two velocity components."""
    dt: float
    dx: float = 1.0 / 32
    band: Optional[float] = None
    interface_radius: int = 1
    sdf_field: str = "dfun"
    velx_field: str = "velx"
    vely_field: str = "vely"

    def __post_init__(self):
        for name in ("dt", "dx"):
            value = getattr(self, name)
            if isinstance(value, bool) or not isinstance(value, (int, float)) or not value > 0:
                raise ValueError(f"{name} must be positive, got {value!r}")
        if self.band is not None and not self.band > 0:
            raise ValueError(f"band must be None or positive, got {self.band!r}")
        if int(self.interface_radius) != self.interface_radius or int(self.interface_radius) < 1:
            raise ValueError(f"interface_radius must be an integer of at least 1, got {self.interface_radius!r}")

    def band_width(self) -> float:
        """The band's half-width: ``band``, or 3 dx."""
        return 3.0 * float(self.dx) if self.band is None else float(self.band)

    def channels(self, fields: Sequence[str]) -> tuple:
        """The (signed-distance, x-velocity, y-velocity) channels among the output fields."""
        fields = list(fields)
        for name in (self.sdf_field, self.velx_field, self.vely_field):
            if name not in fields:
                raise ValueError(f"the flow-consistency rows need the field {name!r} among the output fields {fields}")
        return tuple(fields.index(name) for name in (self.sdf_field, self.velx_field, self.vely_field))


@dataclasses.dataclass
class FlowConsistency:
    """What ``flow_consistency`` returns; every tensor is on the device.  The frame rows keep the leading dims (..., T) of the fields, the pair rows
    are (..., T - 1): row t - 1 is the pair of frames that ends in frame t."""
    divergence_rms: torch.Tensor                    # (..., T)      fp32  RMS of div (u, v) over the bulk-liquid cells; NaN where there is none
    bulk_cells: torch.Tensor                        # (..., T)      int32 their number
    kinetic_energy: torch.Tensor                    # (..., T)      fp32  mean of (u^2 + v^2) / 2 over all cells
    enstrophy: torch.Tensor                         # (..., T)      fp32  mean of vorticity^2 / 2 over the interior cells
    transport_rms: torch.Tensor                     # (..., T - 1)  fp32  RMS of phi_t + u . grad phi over the band cells; NaN where there is none
    interface_speed_rms: torch.Tensor               # (..., T - 1)  fp32  RMS of phi_t alone over them
    transport_cells: torch.Tensor                   # (..., T - 1)  int32 their number

    def transport_ratio(self) -> torch.Tensor:
        """transport_rms / interface_speed_rms: 0 where the velocity explains all of the interface's motion, about 1 or above where it explains
        none.  Never synchronises."""
        return self.transport_rms / self.interface_speed_rms


def flow_consistency(sdf: torch.Tensor, velx: torch.Tensor, vely: torch.Tensor, *, spec: FlowSpec) -> FlowConsistency:
    """Do the signed-distance field and the velocity of (..., T, H, W) frames in physical units agree with each other (``ops.flow_consistency``;
    DESIGN.md section 32)?  Per frame: the RMS divergence of (velx, vely) over the bulk liquid (interior cells with no vapour cell, sdf > 0, in
    their (2 r + 1)^2 window), the mean kinetic energy and the mean enstrophy.  Per pair of consecutive frames: the RMS of the level-set transport
    residual phi_t + u . grad phi (time-centred, central differences) over the interior cells within ``band`` of the interface, and of phi_t alone.
    x runs along W, y along H.  fp64 arithmetic, one rounding, one launch with a workgroup per frame, the same bits on every call and for a
    sequence alone or in a batch; never synchronises."""
    if sdf.dim() < 3 or sdf.shape != velx.shape or sdf.shape != vely.shape:
        raise ValueError(f"flow_consistency expects sdf, velx and vely of one shape (..., T, H, W), got {tuple(sdf.shape)}, {tuple(velx.shape)} "
                         f"and {tuple(vely.shape)}")
    if sdf.numel() < 1:
        raise ValueError(f"flow_consistency needs at least one frame, got {tuple(sdf.shape)}")
    from .. import ops
    _require_gpu(sdf)
    lead, (T, H, W) = tuple(sdf.shape[:-3]), (int(v) for v in sdf.shape[-3:])
    flat = lambda t: t.reshape(-1, T, H, W).contiguous().float()
    phi, u, v = flat(sdf), flat(velx), flat(vely)
    S = phi.shape[0]
    rows = {k: torch.empty((S, T if k in ops._FLOW_FRAME_ROWS else T - 1), dtype=torch.int32 if k.endswith("_cells") else torch.float32,
                           device=phi.device) for k in ops._FLOW_ROWS}
    ops.flow_consistency(phi, u, v, float(spec.dx), float(spec.dt), spec.band_width(), int(spec.interface_radius), **rows)
    return FlowConsistency(**{k: r.reshape(lead + (r.shape[1],)) for k, r in rows.items()})


MAX_ENSEMBLE_MEMBERS = 32             # bf_ensemble_scores' limit: the members of a pixel are held in registers


@dataclasses.dataclass(frozen=True)
class EnsembleSpec:
    """An ensemble rollout (``evaluate_rollouts(..., ensemble=EnsembleSpec(members, std))``): every trajectory is rolled out ``members`` times
    from perturbed copies of its first input clip, and every predicted frame is scored across the members.

    members         2 .. 32 rollouts per trajectory.
    std             a float >= 0, or one per input field, in the units the model sees (after normalisation): the standard deviation of the
                    Gaussian noise added to the first input clip (``add_gaussian_noise``); later steps feed the predictions back unperturbed.
    relative        multiply ``std`` by each input field's standard deviation over the store (``DeviceClipStore.field_std()``).
    seed            the generator's key: the noise of member m of the trajectory from sample s is a pure function of (seed, s, m, element).
    control         member 0 is the unperturbed rollout (its rows are those of the plain call).
    fair            the CRPS' pair term is weighted 1 / (2 M (M - 1)) instead of 1 / (2 M^2): unbiased for the CRPS of the underlying distribution.
    rank_histogram  keep the rank histogram of the truth among the members.
    keep_mean       keep the ensemble mean of every predicted frame (as large as one member's archive)."""
    members: int
    std: Union[float, tuple]
    relative: bool = False
    seed: int = 0
    control: bool = True
    fair: bool = False
    rank_histogram: bool = True
    keep_mean: bool = False

    def __post_init__(self):
        from .noise import NoiseSpec
        m = self.members
        if isinstance(m, bool) or not isinstance(m, int) or not 2 <= m <= MAX_ENSEMBLE_MEMBERS:
            raise ValueError(f"EnsembleSpec: members {m!r} must be an integer from 2 to {MAX_ENSEMBLE_MEMBERS}")
        for name in ("control", "fair", "rank_histogram", "keep_mean"):
            if not isinstance(getattr(self, name), bool):
                raise ValueError(f"EnsembleSpec: {name} {getattr(self, name)!r} must be a bool")
        try:
            noise = NoiseSpec(self.std, self.relative, self.seed)       # std, relative and seed are a NoiseSpec's: one set of rules
        except ValueError as e:
            raise ValueError(str(e).replace("NoiseSpec", "EnsembleSpec")) from None
        object.__setattr__(self, "std", noise.std)

    def sigma(self, channels: int, field_std: Optional[Sequence[float]] = None) -> list:
        """The per-channel standard deviations for a clip of ``channels`` input fields; ``relative`` needs ``field_std`` (one per field)."""
        from .noise import NoiseSpec
        return NoiseSpec(self.std, self.relative, self.seed).sigma(channels, field_std)


@dataclasses.dataclass
class EnsembleScores:
    """What ``ensemble_scores`` returns; every tensor is on the device and keeps the leading dims of the target."""
    mean_rmse: torch.Tensor                         # (...)            fp32  RMSE of the ensemble mean
    spread: torch.Tensor                            # (...)            fp32  sqrt(mean over pixels of the unbiased member variance)
    crps: torch.Tensor                              # (...)            fp32  mean over pixels of the continuous ranked probability score
    rank_hist: Optional[torch.Tensor]               # (..., M + 1)     int32 pixels whose truth has exactly r members strictly below it, or None
    mean: Optional[torch.Tensor]                    # (..., H, W)      fp32  the ensemble mean, or None
    members: int

    def spread_skill(self) -> torch.Tensor:
        """spread * sqrt((M + 1) / M) / mean_rmse: 1 for a reliable ensemble, below 1 for an under-dispersive one.  Never synchronises."""
        return self.spread * math.sqrt((self.members + 1) / self.members) / self.mean_rmse


def ensemble_scores(members: torch.Tensor, target: torch.Tensor, *, fair: bool = False, rank_histogram: bool = True,
                    return_mean: bool = False) -> EnsembleScores:
    """How well the spread of an ensemble matches its error, per frame, on the device (``ops.ensemble_scores``): members
    (..., M, H, W) against target (..., H, W), contiguous fp32 device tensors, 2 <= M <= 32.  Per frame: the RMSE of the member mean, the spread
    (root of the mean unbiased member variance), the CRPS in its pairwise form (``fair``: the pair term over M (M - 1) instead of M^2) and the rank
    histogram of the truth (strictly-below counts).  More than one frame costs one transposing copy of the members: the kernel reads member-major
    blocks.  fp64 arithmetic, one rounding, the same bits on every call and for a frame alone or in a batch; never synchronises.  There is no
    CPU path."""
    from .. import ops
    if not isinstance(members, torch.Tensor) or not isinstance(target, torch.Tensor) or not members.is_cuda or not target.is_cuda:
        raise L.BubbleformerHipError("ensemble_scores runs only on a ROCm GPU (gfx950): got a CPU tensor; there is no CPU fallback")
    if members.dim() < 3 or target.dim() != members.dim() - 1 or tuple(members.shape[:-3]) + tuple(members.shape[-2:]) != tuple(target.shape):
        raise ValueError(f"ensemble_scores expects members (..., M, H, W) and target (..., H, W), got {tuple(members.shape)} and {tuple(target.shape)}")
    if members.dtype != torch.float32 or target.dtype != torch.float32 or not members.is_contiguous() or not target.is_contiguous():
        raise ValueError("ensemble_scores expects contiguous fp32 tensors")
    lead, (M, H, W) = tuple(target.shape[:-2]), members.shape[-3:]
    if not 2 <= M <= MAX_ENSEMBLE_MEMBERS:
        raise ValueError(f"ensemble_scores: {M} members, 2 to {MAX_ENSEMBLE_MEMBERS} are supported")
    F = target.numel() // (H * W) if H * W else 0
    if F < 1:
        raise ValueError(f"ensemble_scores needs at least one frame of at least one pixel, got {tuple(target.shape)}")
    x = members.reshape(F, M, H, W).transpose(0, 1)
    x = x.contiguous() if F > 1 else x.reshape(M, 1, H, W)
    new = lambda dtype, *shape: torch.empty(shape, dtype=dtype, device=x.device)
    rows = {k: new(torch.float32, F) for k in ("mean_rmse", "spread", "crps")}
    if rank_histogram:
        rows["rank_hist"] = new(torch.int32, F, M + 1)
    if return_mean:
        rows["mean"] = new(torch.float32, F, H, W)
    ops.ensemble_scores(x, target.reshape(F, H, W), ops.ensemble_workspace(F, M, H, W, x.device), fair, **rows)
    shaped = {k: (rows[k].reshape(lead + tuple(rows[k].shape[1:])) if k in rows else None) for k in ops._ENSEMBLE_ROWS}
    return EnsembleScores(members=int(M), **shaped)
