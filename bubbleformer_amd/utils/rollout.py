"""Autoregressive rollout kept on the device (reference loop: scripts/inference.py:239-252).

The reference moves every prediction to the host and back (`pred.squeeze(0).detach().cpu()` ... `inp.cuda()`); here the eval
forward is captured once in a HIP graph and replayed per step with the previous prediction copied into the graph's static input,
so a step is one graph launch and the trajectory never leaves HBM.

``evaluate_rollouts`` is the reference's evaluation protocol on top of that (scripts/inference.py:230-266, utils/plot_utils.py:30-34, the
rollout notebook's ``get_eikonal_loss``): many trajectories per forward, the targets read where they lie in a ``DeviceClipStore``, every
score of a step from one pass over the prediction (``bf_rollout_score``), forward and scoring captured together as one graph."""
import dataclasses
import inspect
from typing import Callable, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch


def relative_l2_per_step(pred: torch.Tensor, tgt: torch.Tensor) -> torch.Tensor:
    """LpLoss(d=2, p=2, reduce_dims=[0, 1], reductions=["mean", "mean"]) of scripts/inference.py:230 on (T, C, H, W) clips."""
    num = (pred - tgt).flatten(-2).norm(dim=-1)
    den = tgt.flatten(-2).norm(dim=-1)
    return (num / den).mean(0, keepdim=True).mean(1, keepdim=True).squeeze()


def relative_l2_per_frame(pred: torch.Tensor, tgt: torch.Tensor) -> torch.Tensor:
    """The error-versus-time curves of utils/plot_utils.py:30-33 on (T, C, H, W) clips: (T, C) relative L2 over (H, W), for callers
    without a device store (``evaluate_rollouts`` computes the same on the device, in fp64, against the store's own frames)."""
    return torch.norm(pred - tgt, p=2, dim=(2, 3)) / torch.norm(tgt, p=2, dim=(2, 3))


class GraphedForward:
    """model(x, *extra) in eval / no-grad mode, captured in a HIP graph for one input shape.

    Weights: the captured graph reads the model's PREPARED inference weights (bf16 copies and out-projection folds in a per-model arena,
    ops.trunk_eval) by address.  Before every replay the arena is re-prepared in place if the parameters changed since (torch in-place
    updates, ops.adamw_ / ops.lion_, load_state_dict), so a GraphedForward kept across optimizer steps tracks the live parameters; the
    arena and the scratch buffers the capture saw are pinned for the lifetime of the process (ops.clear_scratch / clear_eval_weights
    release them -- only once the graph is gone)."""

    def __init__(self, model, x: torch.Tensor, *extra: torch.Tensor, warmup: int = 2):
        self.model = model.eval()
        self.static_x = x.clone()
        self.extra = extra
        with torch.no_grad():
            s = torch.cuda.Stream()
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):
                for _ in range(warmup):
                    self.model(self.static_x, *extra)
            torch.cuda.current_stream().wait_stream(s)
            self.graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.graph):
                self.static_out = self.model(self.static_x, *extra)

    def __call__(self, x: torch.Tensor) -> torch.Tensor:
        self.static_x.copy_(x)
        owner = self.model.__dict__.get("_bf_eval_owner")
        if owner is not None:
            from .. import ops
            ops.refresh_eval_weights(owner)
        self.graph.replay()
        return self.static_out


def autoregressive_rollout(model, first_input: torch.Tensor, steps: int, *extra: torch.Tensor, use_graph: bool = True,
                           target_fn: Optional[Callable[[int], torch.Tensor]] = None) -> Tuple[torch.Tensor, List[torch.Tensor]]:
    """first_input (T, C, H, W) on the device; each step feeds the previous prediction back (scripts/inference.py:242-245).
    Returns (predictions concatenated along time: (steps*T, C, H, W), per-step relative L2 against target_fn(step) if given)."""
    x = first_input.unsqueeze(0).float()
    fwd = GraphedForward(model, x, *extra) if use_graph else None
    preds, errs = [], []
    with torch.no_grad():
        for s in range(steps):
            out = fwd(x) if fwd is not None else model.eval()(x, *extra)
            pred = out.squeeze(0).clone()
            preds.append(pred)
            if target_fn is not None:
                errs.append(relative_l2_per_step(pred, target_fn(s)))
            x = pred.unsqueeze(0)
    return torch.cat(preds, dim=0), errs


class RolloutPlan(NamedTuple):
    first: List[int]                # absolute first input frame of step 0 on the store's frame axis, per trajectory
    files: List[int]                # file of every trajectory
    timesteps: torch.Tensor         # (B, steps*T) int64: frame number inside its file of every predicted frame (scripts/inference.py:251)


def plan_rollouts(dataset, starts: Sequence[int], steps: int, model_time_window: Optional[int] = None) -> RolloutPlan:
    """The host side of ``evaluate_rollouts``, without a GPU: trajectory b starts with the input clip of ``dataset[starts[b]]`` and is scored
    at step s against the target clip of ``dataset[starts[b] + s * T]`` (`for itr in range(0, n, T)` of scripts/inference.py:239-252), so
    every one of those samples must exist in the file of ``starts[b]``."""
    T = int(dataset.time_window)
    if list(dataset.input_fields) != list(dataset.output_fields):
        raise ValueError(f"a rollout feeds predictions back as inputs: input fields {list(dataset.input_fields)} and output fields "
                         f"{list(dataset.output_fields)} must be the same")
    if int(steps) < 1:
        raise ValueError("steps must be at least 1")
    if model_time_window is not None and int(model_time_window) != T:
        raise ValueError(f"the model was built for time_window = {model_time_window}, the dataset has {T}")
    if len(starts) < 1:
        raise ValueError("at least one trajectory")
    ends = np.cumsum(dataset._per_traj())               # one past the last sample of every file
    frame0 = np.concatenate([[0], np.cumsum(dataset.traj_lens)])
    first, files, times = [], [], []
    for b, idx in enumerate(starts):
        idx = int(idx)
        if idx < 0 or idx >= len(dataset):
            raise IndexError(f"trajectory {b}: sample {idx} is outside the dataset (0 .. {len(dataset) - 1})")
        fi, start = dataset.locate(idx)
        fit = (int(ends[fi]) - 1 - idx) // T + 1        # steps whose target sample is still in this file
        if steps > fit:
            raise IndexError(f"trajectory {b} (sample {idx}, file {fi}): step {fit} is the last that fits, {steps} were asked for")
        first.append(int(frame0[fi]) + start)
        files.append(fi)
        times.append(torch.arange(start + T, start + T + steps * T, dtype=torch.int64))
    return RolloutPlan(first, files, torch.stack(times))


@dataclasses.dataclass
class RolloutReport:
    """What ``evaluate_rollouts`` returns; every tensor is on the device.  Row s * T + t of the frame axis is frame t of step s."""
    rel_l2: torch.Tensor                            # (B, steps*T, C)  relative L2 per predicted frame and field (plot_utils.py:30-33)
    criterion: torch.Tensor                         # (B, steps)       their mean per step (the LpLoss scripts/inference.py:252 prints)
    eikonal_pred: Optional[torch.Tensor]            # (B, steps*T)     the notebook's Eikonal score of the predicted interface, or None
    eikonal_target: Optional[torch.Tensor]          # (B, steps*T)     the same of the simulated one
    timesteps: torch.Tensor                         # (B, steps*T)     int64 frame numbers inside the trajectory's file
    fields: List[str]                               # output field names in channel order
    predictions: Optional[torch.Tensor] = None      # (B, steps*T, C, Ho, Wo) if kept
    heatflux_pred: Optional[torch.Tensor] = None    # (B, steps*T)     heater heat flux of every predicted frame (utils/heatflux.py), or None
    heatflux_target: Optional[torch.Tensor] = None  # (B, steps*T)     the same of the simulated one
    bubble_count_pred: Optional[torch.Tensor] = None        # (B, steps*T) int32   bubbles of every predicted frame (physics.bubble_census), or None
    bubble_count_target: Optional[torch.Tensor] = None      # (B, steps*T) int32   the same of the simulated one
    bubble_attached_pred: Optional[torch.Tensor] = None     # (B, steps*T) int32   those with a cell in the heater row
    bubble_attached_target: Optional[torch.Tensor] = None
    vapour_fraction_pred: Optional[torch.Tensor] = None     # (B, steps*T) fp32    vapour cells / all cells
    vapour_fraction_target: Optional[torch.Tensor] = None
    bubble_area_pred: Optional[torch.Tensor] = None         # (B, steps*T, max_bubbles) int32 cells, in raster order of the first cell, then 0
    bubble_area_target: Optional[torch.Tensor] = None
    bubble_dx: Optional[float] = None                       # the cell size of the census' BubbleSpec (for the equivalent diameters)
    # with BubbleSpec(track=True): row s * T + t - 1 is the pair of frames that ends in frame t of step s (physics.bubble_tracks), else None
    bubble_events_pred: Optional[torch.Tensor] = None           # (B, steps*T-1, 5) int32   births, deaths, merges, splits, departures
    bubble_events_target: Optional[torch.Tensor] = None
    bubble_successor_pred: Optional[torch.Tensor] = None        # (B, steps*T-1, max_bubbles) int32
    bubble_successor_target: Optional[torch.Tensor] = None
    bubble_predecessor_pred: Optional[torch.Tensor] = None      # (B, steps*T-1, max_bubbles) int32
    bubble_predecessor_target: Optional[torch.Tensor] = None
    bubble_departure_area_pred: Optional[torch.Tensor] = None   # (B, steps*T-1, max_bubbles) int32 cells of a bubble that leaves the heater, else 0
    bubble_departure_area_target: Optional[torch.Tensor] = None
    # with BubbleSpec(match=True): row s * T + t is the predicted frame t of step s against the simulated one (physics.bubble_match), else None.
    # Attributes that evaluate_rollouts sets, as the error rows below and for the same reason
    bubble_match_pred = None                            # (B, steps*T, max_bubbles) int32   the simulated bubble matched to predicted bubble k + 1, or 0
    bubble_match_target = None                          # (B, steps*T, max_bubbles) int32   the predicted bubble matched to simulated bubble k + 1, or 0
    bubble_match_overlap = None                         # (B, steps*T, max_bubbles) int32   cells the matched pair shares, at the predicted bubble's slot
    bubble_match_displacement = None                    # (B, steps*T, max_bubbles) fp32    distance between the pair's centroids, in cells
    bubble_match_counts = None                          # (B, steps*T, 6) int32   hits, misses, false alarms; the same three for bubbles on the heater
    bubble_mask_cells = None                            # (B, steps*T, 2) int32   cells vapour on both sides, on either
    # with errors=ErrorSpec(): e = prediction - target in fp64 (physics.field_errors), else None.  Attributes that evaluate_rollouts sets, not
    # constructor arguments: the dataclass fields end at the tracking rows, so positional callers and dataclasses.fields() stay as they are
    rmse = None                                         # (B, steps*T, C)     fp32 sqrt(mean e^2)
    max_error = None                                    # (B, steps*T, C)     fp32 max |e|
    boundary_rmse = None                                # (B, steps*T, C)     fp32 the root mean square over the outer ring of cells
    interface_rmse = None                               # (B, steps*T, C)     fp32 the same over the interface cells of the simulated frame
    interface_cells = None                              # (B, steps*T, C)     int32 their number (one mask for all C channels)
    spectral_error = None                               # (B, steps*T, C, 3)  fp32 band-limited RMSE of e: low, mid, high (ErrorSpec(spectra=True))
    spectrum_error = None                               # (B, steps*T, C, K)  fp32 shell power of e
    spectrum_pred = None                                # (B, steps*T, C, K)  fp32 shell power of the prediction
    spectrum_target = None                              # (B, steps*T, C, K)  fp32 shell power of the target
    # with ensemble=EnsembleSpec(M, ...): B = M * Bt rows above, member-major (row m * Bt + b is member m of trajectory b), and the statistics across
    # the members (physics.ensemble_scores) per trajectory, else None.  Attributes as the error rows are, for the same reason
    ensemble_members = None                             # M
    ensemble_mean_rmse = None                           # (Bt, steps*T, C)         fp32 RMSE of the member mean
    ensemble_spread = None                              # (Bt, steps*T, C)         fp32 sqrt(mean unbiased member variance)
    ensemble_crps = None                                # (Bt, steps*T, C)         fp32 mean CRPS over the pixels
    ensemble_rank_hist = None                           # (Bt, steps*T, C, M + 1)  int32 pixels whose truth has r members strictly below it
    ensemble_mean = None                                # (Bt, steps*T, C, Ho, Wo) fp32 the member mean (EnsembleSpec(keep_mean=True))
    # from evaluate_rollouts_redistanced: the status and the change of the correction of every predicted frame (physics.redistance), else None
    redistance_rounds = None                            # (B, steps*T)        int32 passes run; 0 one sign or a skipped step, -1 non-finite, -2 ran out
    redistance_change = None                            # (B, steps*T)        fp32 root mean square change of the physical field
    # from evaluate_rollouts_flow: do the signed distance and the velocity of one side agree with each other (physics.flow_consistency), else None.
    # The *_target rows are the SIMULATION's own residuals, the baseline to read the prediction's against: they are not zero, since the frames are
    # stored at a coarse interval and boiling moves the interface relative to the fluid.  Attributes as the error rows are, for the same reason
    flow_divergence_pred = None                         # (B, steps*T)        fp32 RMS divergence of the velocity over the bulk-liquid cells
    flow_divergence_target = None
    flow_bulk_cells_pred = None                         # (B, steps*T)        int32 their number
    flow_bulk_cells_target = None
    flow_kinetic_energy_pred = None                     # (B, steps*T)        fp32 mean (u^2 + v^2) / 2
    flow_kinetic_energy_target = None
    flow_enstrophy_pred = None                          # (B, steps*T)        fp32 mean vorticity^2 / 2 over the interior cells
    flow_enstrophy_target = None
    flow_transport_pred = None                          # (B, steps*T-1)      fp32 RMS of phi_t + u . grad phi near the interface; row s * T + t - 1 is the pair that ends in frame t of step s
    flow_transport_target = None
    flow_interface_speed_pred = None                    # (B, steps*T-1)      fp32 RMS of phi_t alone over the same cells
    flow_interface_speed_target = None
    flow_transport_cells_pred = None                    # (B, steps*T-1)      int32 their number
    flow_transport_cells_target = None
    flow_dx = None                                      # the FlowSpec's cell size and time between frames
    flow_dt = None

    def _flow(self):
        if self.flow_divergence_pred is None:
            raise ValueError("this report has no flow-consistency rows: call evaluate_rollouts_flow(..., FlowSpec(dt))")

    def transport_ratio(self) -> Tuple[torch.Tensor, torch.Tensor]:
        """(prediction, simulation): (B, steps*T-1) fp32 flow_transport / flow_interface_speed of a side, 0 where its velocity explains all of its
        interface's motion, about 1 or above where it explains none.  Read the prediction's against the simulation's, not against zero.  On the
        device; never synchronises."""
        self._flow()
        return self.flow_transport_pred / self.flow_interface_speed_pred, self.flow_transport_target / self.flow_interface_speed_target

    def energy_drift(self) -> torch.Tensor:
        """(B, steps*T) fp32: flow_kinetic_energy_pred / flow_kinetic_energy_target, 1 for a prediction that keeps the flow's energy.  On the
        device; never synchronises."""
        self._flow()
        return self.flow_kinetic_energy_pred / self.flow_kinetic_energy_target

    def divergence_excess(self) -> torch.Tensor:
        """(B, steps*T) fp32: flow_divergence_pred / flow_divergence_target, how much more compressible the predicted bulk liquid is than the
        simulated one on the same stencil.  On the device; never synchronises."""
        self._flow()
        return self.flow_divergence_pred / self.flow_divergence_target

    def _ensemble(self):
        if self.ensemble_members is None:
            raise ValueError("this report has no ensemble rows: call evaluate_rollouts(..., ensemble=EnsembleSpec(members, std))")
        return int(self.ensemble_members)

    def by_member(self, t: torch.Tensor) -> torch.Tensor:
        """A per-member tensor of the report (M * Bt, ...) as a view (M, Bt, ...)."""
        M = self._ensemble()
        return t.view(M, t.shape[0] // M, *t.shape[1:])

    def spread_skill(self) -> torch.Tensor:
        """(Bt, steps*T, C) fp32: ensemble_spread * sqrt((M + 1) / M) / ensemble_mean_rmse, 1 for a reliable ensemble (below 1: the members
        agree more than their mean is right).  On the device; never synchronises."""
        M = self._ensemble()
        return self.ensemble_spread * float(np.sqrt((M + 1) / M)) / self.ensemble_mean_rmse

    def rank_histogram(self) -> torch.Tensor:
        """(Bt, C, M + 1) int64: the rank histogram summed over the frames (flat for a reliable ensemble, U-shaped for an under-dispersive
        one).  On the device; never synchronises."""
        self._ensemble()
        if self.ensemble_rank_hist is None:
            raise ValueError("this report kept no rank histogram: use EnsembleSpec(rank_histogram=True)")
        return self.ensemble_rank_hist.sum(dim=1, dtype=torch.int64)

    def save(self, path) -> None:
        """``torch.save`` of the report's tensors, in the spirit of scripts/inference.py:265."""
        out = {"timesteps": self.timesteps, "rel_l2": self.rel_l2, "criterion": self.criterion, "fields": list(self.fields)}
        if self.predictions is not None:
            out["preds"] = self.predictions
        if self.eikonal_pred is not None:
            out["eikonal_pred"], out["eikonal_target"] = self.eikonal_pred, self.eikonal_target
        if self.heatflux_pred is not None:
            out["heatflux_pred"], out["heatflux_target"] = self.heatflux_pred, self.heatflux_target
        if self.bubble_count_pred is not None:
            for key in _BUBBLE_KEYS:
                out[key] = getattr(self, key)
        if self.bubble_events_pred is not None:
            for key in _TRACK_KEYS:
                out[key] = getattr(self, key)
        for key in _MATCH_KEYS + _ERROR_KEYS + _ENSEMBLE_KEYS + _REDISTANCE_KEYS + _FLOW_KEYS:
            if getattr(self, key) is not None:
                out[key] = getattr(self, key)
        torch.save(out, path)

    def spectral_ratio(self) -> torch.Tensor:
        """(B, steps*T, C, K) fp32: spectrum_pred / spectrum_target per shell, the blurring curve (below 1 where the prediction lost power; inf
        or NaN where the simulation has none).  On the device; never synchronises."""
        if self.spectrum_pred is None:
            raise ValueError("this report has no spectra: call evaluate_rollouts(..., errors=ErrorSpec(spectra=True))")
        return self.spectrum_pred / self.spectrum_target

    def _heatfluxes(self):
        if self.heatflux_pred is None:
            raise ValueError("this report has no heat-flux rows: call evaluate_rollouts(..., heatflux=HeaterSpec(...))")
        return self.heatflux_target, self.heatflux_pred

    def heatflux_kl(self, points: int = 1000, pooled: bool = False) -> torch.Tensor:
        """KL(simulation || model) of the heat-flux distributions (examples/data_visualization.ipynb cell 4, ``physics.kde_kl_divergence``):
        (B,) per trajectory, or with ``pooled`` the one divergence of all trajectories' rows together -- the notebook's number for one long
        series.  On the device; the caller synchronises when it reads the value."""
        from .physics import kde_kl_divergence
        sim, model = self._heatfluxes()
        return kde_kl_divergence(sim.reshape(-1), model.reshape(-1), points) if pooled else kde_kl_divergence(sim, model, points)

    def save_heatfluxes(self, path) -> None:
        """The file examples/data_visualization.ipynb cell 2 loads: {"sim_hf", "model_hf"} as 1-D CPU float tensors, all trajectories in order."""
        sim, model = self._heatfluxes()
        torch.save({"sim_hf": sim.reshape(-1).float().cpu(), "model_hf": model.reshape(-1).float().cpu()}, path)

    def _bubbles(self):
        if self.bubble_count_pred is None:
            raise ValueError("this report has no bubble census: call evaluate_rollouts(..., bubbles=BubbleSpec(...))")

    def vapour_drift(self) -> torch.Tensor:
        """(B, steps*T) fp32: (predicted - simulated) / simulated vapour fraction of every frame, the mass-conservation curve (inf or NaN
        where the simulated frame has no vapour).  On the device; never synchronises."""
        self._bubbles()
        return (self.vapour_fraction_pred - self.vapour_fraction_target) / self.vapour_fraction_target

    def bubble_diameters(self, dx: Optional[float] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """(simulation, model): the equivalent diameters 2 * sqrt(area * dx^2 / pi) of all recorded bubbles of all frames and trajectories, each
        a 1-D fp32 device tensor in report order.  SYNCHRONISES: dropping the empty slots makes the host wait for their number."""
        from .physics import equivalent_diameter
        self._bubbles()
        dx = self.bubble_dx if dx is None else dx
        return tuple(equivalent_diameter(a[a > 0], dx) for a in (self.bubble_area_target, self.bubble_area_pred))

    def bubble_size_kl(self, points: int = 1000) -> torch.Tensor:
        """KL(simulation || model) of the bubble-size distributions: ``physics.kde_kl_divergence`` of ``bubble_diameters()``, a 0-d fp64 device
        tensor.  NaN when either side has fewer than two recorded bubbles (a model that predicts no vapour: a density needs two samples), as
        it is for a side whose bubbles all have one size.  Synchronises as ``bubble_diameters`` does."""
        from .physics import kde_kl_divergence
        sim, model = self.bubble_diameters()
        if sim.numel() < 2 or model.numel() < 2:
            return torch.full((), float("nan"), dtype=torch.float64, device=sim.device)
        return kde_kl_divergence(sim, model, points)


    def _tracks(self):
        if self.bubble_events_pred is None:
            raise ValueError("this report has no bubble tracking: call evaluate_rollouts(..., bubbles=BubbleSpec(track=True))")

    def bubble_track_ids(self) -> Tuple[Tuple[torch.Tensor, torch.Tensor], Tuple[torch.Tensor, torch.Tensor]]:
        """((track_id, n_tracks) of the simulation, the same of the model): track_id (B, steps*T, max_bubbles) and n_tracks (B,) int32, every
        trajectory one sequence (``ops.bubble_track_ids``, one launch per side, after the rollout).  On the device; never synchronises."""
        from .. import ops
        self._tracks()
        out = []
        for count, succ, pred in ((self.bubble_count_target, self.bubble_successor_target, self.bubble_predecessor_target),
                                  (self.bubble_count_pred, self.bubble_successor_pred, self.bubble_predecessor_pred)):
            B, F = count.shape
            ids = torch.empty((B, F, succ.shape[-1]), dtype=torch.int32, device=count.device)
            n = torch.empty(B, dtype=torch.int32, device=count.device)
            ops.bubble_track_ids(count, succ, pred, ids, n)
            out.append((ids, n))
        return tuple(out)

    def departure_diameters(self, dx: Optional[float] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """(simulation, model): the equivalent diameters of the bubbles that leave the heater, each a 1-D fp32 device tensor in report order.
        SYNCHRONISES, as ``bubble_diameters`` does."""
        from .physics import departure_diameters
        self._tracks()
        dx = self.bubble_dx if dx is None else dx
        return departure_diameters(self.bubble_departure_area_target, dx), departure_diameters(self.bubble_departure_area_pred, dx)

    def departure_frequency(self) -> Tuple[torch.Tensor, torch.Tensor]:
        """(simulation, model): (B,) fp64 departures per frame pair of every trajectory.  On the device; never synchronises."""
        from .physics import departure_frequency
        self._tracks()
        return departure_frequency(self.bubble_events_target), departure_frequency(self.bubble_events_pred)

    def departure_diameter_kl(self, points: int = 1000) -> torch.Tensor:
        """KL(simulation || model) of the departure-diameter distributions: ``physics.kde_kl_divergence`` of ``departure_diameters()``, a 0-d fp64
        device tensor; NaN when either side has fewer than two departures, as ``bubble_size_kl``.  Synchronises as ``departure_diameters`` does."""
        from .physics import kde_kl_divergence
        sim, model = self.departure_diameters()
        if sim.numel() < 2 or model.numel() < 2:
            return torch.full((), float("nan"), dtype=torch.float64, device=sim.device)
        return kde_kl_divergence(sim, model, points)

    def _matches(self):
        if self.bubble_match_counts is None:
            raise ValueError("this report has no bubble matching: call evaluate_rollouts(..., bubbles=BubbleSpec(match=True))")

    def bubble_detection(self, attached: bool = False) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """(precision, recall, critical success index) against lead time, each (B, steps*T) fp32: hits / (hits + false alarms), hits / (hits +
        misses), hits / (hits + misses + false alarms) of every frame's bubbles, or with ``attached`` of those on the heater; NaN where the
        denominator is 0 (``physics.detection_scores``).  On the device; never synchronises."""
        from .physics import detection_scores
        self._matches()
        return detection_scores(self.bubble_match_counts, attached)

    def mask_iou(self) -> torch.Tensor:
        """(B, steps*T) fp32: the IoU of the predicted and the simulated vapour mask of every frame, NaN where neither has vapour."""
        from .physics import mask_iou
        self._matches()
        return mask_iou(self.bubble_mask_cells)

    def matched_iou(self) -> torch.Tensor:
        """(B, steps*T, max_bubbles) fp32: the IoU of every matched pair at the predicted bubble's slot, NaN elsewhere."""
        from .physics import matched_iou
        self._matches()
        return matched_iou(self.bubble_match_overlap, self.bubble_match_pred, self.bubble_area_pred, self.bubble_area_target)

    def centroid_error(self, dx: Optional[float] = None) -> torch.Tensor:
        """(B, steps*T) fp32: the mean centroid displacement of every frame's matched pairs times ``dx`` (default: the census' cell size), NaN
        where a frame has no matched pair."""
        from .physics import centroid_error
        self._matches()
        return centroid_error(self.bubble_match_displacement, self.bubble_match_pred, self.bubble_dx if dx is None else dx)


_TRACK_KEYS = ("bubble_events_pred", "bubble_events_target", "bubble_successor_pred", "bubble_successor_target", "bubble_predecessor_pred",
               "bubble_predecessor_target", "bubble_departure_area_pred", "bubble_departure_area_target")
_MATCH_KEYS = ("bubble_match_pred", "bubble_match_target", "bubble_match_overlap", "bubble_match_displacement", "bubble_match_counts",
               "bubble_mask_cells")
_ERROR_KEYS = ("rmse", "max_error", "boundary_rmse", "interface_rmse", "interface_cells", "spectral_error", "spectrum_error", "spectrum_pred",
               "spectrum_target")
_ENSEMBLE_KEYS = ("ensemble_members", "ensemble_mean_rmse", "ensemble_spread", "ensemble_crps", "ensemble_rank_hist", "ensemble_mean")
_REDISTANCE_KEYS = ("redistance_rounds", "redistance_change")
# report attribute -> member of bf_flow_rows, per side
_FLOW_ROW_NAMES = {"flow_divergence": "divergence_rms", "flow_bulk_cells": "bulk_cells", "flow_kinetic_energy": "kinetic_energy", "flow_enstrophy": "enstrophy",
                   "flow_transport": "transport_rms", "flow_interface_speed": "interface_speed_rms", "flow_transport_cells": "transport_cells"}
_FLOW_KEYS = tuple(f"{name}_{side}" for name in _FLOW_ROW_NAMES for side in ("pred", "target")) + ("flow_dx", "flow_dt")
_BUBBLE_KEYS = ("bubble_count_pred", "bubble_count_target", "bubble_attached_pred", "bubble_attached_target", "vapour_fraction_pred",
                "vapour_fraction_target", "bubble_area_pred", "bubble_area_target")


def _to_device(values, dtype, device) -> torch.Tensor:
    host = torch.as_tensor(values, dtype=dtype)
    return host.pin_memory().to(device, non_blocking=True) if device.type == "cuda" else host.to(device)


def _frames_store(data, device):
    """``data`` as the store whose fp32 frames the rollout kernels read where they lie: a DeviceClipStore, or a dataset's.  A store in
    another storage form is refused -- its ``to_fp32()`` is what to pass."""
    from ..data.dataset import DeviceClipStore
    store = data if isinstance(data, DeviceClipStore) else data.device_store(device)
    if store.storage != "fp32":
        raise ValueError(f"rollout evaluation reads stored fp32 frames inside its kernels and this store's storage is {store.storage!r}: pass store.to_fp32()")
    return store


def evaluate_rollouts(model, data, starts: Sequence[int], steps: int, *, use_graph: bool = True, sdf_field: Optional[str] = "dfun",
                      keep_predictions: bool = False, heatflux: "Optional[HeaterSpec]" = None,  # noqa: F821 (physics.HeaterSpec)
                      bubbles: "Optional[BubbleSpec]" = None,  # noqa: F821 (physics.BubbleSpec)
                      errors: "Optional[ErrorSpec]" = None,  # noqa: F821 (physics.ErrorSpec)
                      ensemble: "Optional[EnsembleSpec]" = None) -> RolloutReport:  # noqa: F821 (physics.EnsembleSpec)
    """Roll ``model`` out over ``B = len(starts)`` test trajectories at once and score every predicted frame against the simulation.

    data: a ``BubbleForecast`` (its device store is made on the model's device) or a ``DeviceClipStore``; starts: dataset sample indices.
    A step is the eval forward on the batch of B clips followed by ONE scoring call (``ops.rollout_score``) that reads the prediction once,
    takes its targets from the store, writes that step's rows of the report, the next step's input and, if kept, the archive, and advances
    a step counter that lives on the device.  With ``use_graph`` both are captured as one linear HIP graph and replayed ``steps`` times with
    no other host work between replays; without, the same two calls run eagerly and give the same bits.  A model whose ``forward`` takes
    ``fluid_params`` gets the store's fluid row of each trajectory's file.  With ``heatflux`` (a ``physics.HeaterSpec``) the step also leaves
    the heater heat flux of every predicted and simulated frame (``ops.rollout_heatflux``, issued right before the scoring call and captured
    with it); ``None`` leaves the launches and the report as they are without it.  With ``bubbles`` (a ``physics.BubbleSpec``) the step
    likewise leaves the bubble census of every predicted and simulated frame (``ops.rollout_bubbles``, one more launch before the scoring
    call): the ``bubble_*`` and ``vapour_fraction_*`` rows of the report; with ``BubbleSpec(track=True)`` that launch also leaves its label
    images and one more (``ops.rollout_bubble_links``) follows the bubbles into this step's frames: the ``bubble_events_*``, ``bubble_successor_*``,
    ``bubble_predecessor_*`` and ``bubble_departure_area_*`` rows; with ``BubbleSpec(match=True)`` one more (``ops.rollout_bubble_match``) matches
    the predicted bubbles of every frame of the step to the simulated ones: the ``bubble_match_*`` and ``bubble_mask_cells`` rows, which
    ``report.bubble_detection()``, ``mask_iou()``, ``matched_iou()`` and ``centroid_error()`` read.  With ``errors`` (a ``physics.ErrorSpec``) one more call before the scoring
    call (``ops.rollout_errors``) leaves ``physics.field_errors``' rows of every predicted frame and field against the stored target: ``rmse``,
    ``max_error``, ``boundary_rmse``, the interface rows when the signed-distance field is among the outputs, and with ``spectra`` the shell
    spectra and the band-limited errors; ``None`` leaves the launches and the report as they are without it.  Never synchronises.

    With ``ensemble`` (a ``physics.EnsembleSpec`` of M members) the call is the plain call on ``list(starts) * M`` -- every row of the report,
    the heat-flux, bubble and error rows included, is then per member, (M * Bt, ...) member-major, ``report.by_member(t)`` views it as
    (M, Bt, ...), and ``render_rollouts(report, data, list(starts) * M, ...)`` draws it -- plus two things.  After the input gather, member m's
    block of the first input clips is perturbed in place by one ``add_gaussian_noise`` launch with ``draw=m`` and the trajectories' sample
    numbers as ids (member 0 stays as gathered with ``control``): the noise of member m of the trajectory from sample s is a pure function of
    (seed, s, m, element), whatever the other trajectories, Bt or M of the call.  And one more call before the scoring call
    (``ops.rollout_ensemble``, captured with it) leaves the statistics across the members of every predicted frame and field:
    ``ensemble_mean_rmse``, ``ensemble_spread``, ``ensemble_crps`` (Bt, steps*T, C), ``ensemble_rank_hist`` and, if kept, ``ensemble_mean``;
    ``report.spread_skill()`` and ``report.rank_histogram()`` read them.  ``EnsembleSpec(relative=True)`` takes ``store.field_std()`` first,
    which is ONE host synchronisation before the loop; nothing else of the call waits for the device.

    ``evaluate_rollouts_redistanced`` is this call with the predicted signed-distance field redistanced in place at the head of every step,
    ``evaluate_rollouts_flow`` this call with the flow-consistency rows of both sides."""
    return _evaluate_rollouts(model, data, starts, steps, None, use_graph=use_graph, sdf_field=sdf_field, keep_predictions=keep_predictions,
                              heatflux=heatflux, bubbles=bubbles, errors=errors, ensemble=ensemble)


def evaluate_rollouts_redistanced(model, data, starts: Sequence[int], steps: int, redistance: "Optional[RedistanceSpec]",  # noqa: F821 (physics.RedistanceSpec)
                                  **options) -> RolloutReport:
    """``evaluate_rollouts(model, data, starts, steps, **options)`` with the predicted signed-distance field repaired as the rollout goes.

    With ``redistance`` (a ``physics.RedistanceSpec``) the FIRST call of a step, before every other call of it, replaces the signed-distance channel of the
    prediction in place by its redistanced field (``ops.rollout_redistance``: de-normalised, ``physics.redistance``, renormalised), on the steps s
    with (s + 1) % every == 0: the heat flux, the census, the errors, the ensemble statistics and the scores all see the corrected prediction, and the
    scoring call feeds it back and archives it.  The report gains ``redistance_rounds`` and ``redistance_change`` (B, steps*T), per member with
    ``ensemble``.  ``redistance=None`` is ``evaluate_rollouts`` itself: the same launches, the same bits.  The operation is first order and not differentiable: it
    belongs to evaluation, not to ``autoregressive_rollout`` or the training step.

    A function of its own rather than one more keyword of ``evaluate_rollouts``: that function's parameter list is held as it is."""
    return _evaluate_rollouts(model, data, starts, steps, redistance, **options)


def evaluate_rollouts_flow(model, data, starts: Sequence[int], steps: int, flow: "Optional[FlowSpec]", **options) -> RolloutReport:  # noqa: F821 (physics.FlowSpec)
    """``evaluate_rollouts(model, data, starts, steps, **options)`` plus the question whether the fields of ONE prediction agree with each other.

    With ``flow`` (a ``physics.FlowSpec``; its ``dt`` is the time between two stored frames) one more call before the scoring call
    (``ops.rollout_flow``, captured with it) leaves ``physics.flow_consistency``'s rows of every frame and of every pair of consecutive frames,
    for the de-normalised prediction and for the simulation: ``flow_divergence_*``, ``flow_bulk_cells_*``, ``flow_kinetic_energy_*`` and
    ``flow_enstrophy_*`` (B, steps*T), ``flow_transport_*``, ``flow_interface_speed_*`` and ``flow_transport_cells_*`` (B, steps*T-1), where row
    s * T + t - 1 is the pair that ends in frame t of step s -- pairs across a step boundary included; the pair from the last input frame to the
    first predicted one is not scored.  The ``*_target`` rows are the simulation's own residuals and are NOT zero: the frames are stored at a
    coarse interval, and boiling moves the interface relative to the fluid.  They are the baseline: ``report.transport_ratio()``,
    ``energy_drift()`` and ``divergence_excess()`` set the prediction against them.  ``options`` are ``evaluate_rollouts``' keywords plus
    ``redistance=`` (a ``physics.RedistanceSpec``, as ``evaluate_rollouts_redistanced`` takes it): the flow call is issued after the correction, so
    the rows are those of the corrected signed distance.  With ``ensemble=`` the rows are per member.  ``flow=None`` is the call without it: the
    same launches, the same bits.  Never synchronises.

    A function of its own rather than one more keyword of ``evaluate_rollouts``: that function's parameter list is held as it is."""
    redistance = options.pop("redistance", None)
    return _evaluate_rollouts(model, data, starts, steps, redistance, flow=flow, **options)


def _evaluate_rollouts(model, data, starts, steps, redistance, *, use_graph=True, sdf_field="dfun", keep_predictions=False, heatflux=None, bubbles=None,
                       errors=None, ensemble=None, flow=None) -> RolloutReport:
    """The one implementation behind ``evaluate_rollouts`` (redistance = None), ``evaluate_rollouts_redistanced`` and ``evaluate_rollouts_flow``."""
    from .. import ops
    device = next(model.parameters()).device
    store = _frames_store(data, device)
    ds = store.ds
    members = None
    if ensemble is not None:
        members, trajectories = int(ensemble.members), [int(i) for i in starts]
        starts = trajectories * members                 # member-major: row m * Bt + b is member m of trajectory b
    plan = plan_rollouts(ds, starts, steps, getattr(model, "time_window", None))
    if store.frames.device != device:
        raise ValueError(f"the store is on {store.frames.device}, the model on {device}")
    B, T, f = len(plan.first), int(ds.time_window), int(ds.downsample_factor)
    Ho, Wo = (store.H // f, store.W // f) if f > 1 else (store.H, store.W)
    fields = list(ds.output_fields)
    sdf = fields.index(sdf_field) if sdf_field in fields else -1
    extra = ()
    if "fluid_params" in inspect.signature(model.forward).parameters:
        if store.fluid is None:
            raise ValueError("the model is conditioned on fluid parameters; build the dataset with return_fluid_params=True")
        extra = (store.fluid[_to_device(plan.files, torch.int64, device)],)
    first = _to_device(plan.first, torch.int64, device)
    x = ops.clip_gather(store.frames, first, 0, T, store.in_tab, Ho, Wo)          # the input clips of data[starts[b]], as gather() builds them
    C = len(fields)
    new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=device)
    if members is not None:
        from .noise import add_gaussian_noise, stage_sample_ids
        Bt = len(trajectories)
        field_std = None
        if ensemble.relative:                           # the one host synchronisation of an ensemble call
            by_name = store.field_std()
            field_std = [by_name[name] for name in ds.input_fields]
        sigma = ensemble.sigma(x.shape[2], field_std)
        if any(v > 0.0 for v in sigma):
            sigma = torch.tensor(sigma, dtype=torch.float32).pin_memory().to(device, non_blocking=True)
            ids = stage_sample_ids(trajectories, Bt, device)
            for m in range(1 if ensemble.control else 0, members):
                block = x[m * Bt:(m + 1) * Bt]
                add_gaussian_noise(block, sigma, sample_ids=ids, draw=m, pass_index=0, seed=ensemble.seed, out=block)
    rel_l2, criterion = new(B, steps * T, C), new(B, steps)
    eik_p, eik_t = (new(B, steps * T), new(B, steps * T)) if sdf >= 0 else (None, None)
    archive = new(B, steps * T, C, Ho, Wo) if keep_predictions else None
    counter = torch.zeros(1, dtype=torch.int32, device=device)
    ws = ops.rollout_score_workspace(x)
    before_score = []                               # (pred, step) calls that read the step counter the scoring call then advances, in launch order
    red_rows = None
    if redistance is not None:                      # first: every later call of the step reads the corrected prediction
        red_args = (redistance.channel(fields), steps, float(redistance.dx), redistance.band, redistance.max_rounds, int(redistance.every),
                    ops.redistance_workspace(B * T, Ho, Wo, device))
        red_rows = (torch.empty((B, steps * T), dtype=torch.int32, device=device), new(B, steps * T))
        before_score.append(lambda pred, step: ops.rollout_redistance(pred, store.frames, first, step, store.out_tab, *red_args, *red_rows))
    flow_rows = None
    if flow is not None:                            # right behind the correction: the rows are those of the corrected signed distance
        flow_channels = flow.channels(fields)
        flow_rows = [{k: torch.empty((B, steps * T if k in ops._FLOW_FRAME_ROWS else steps * T - 1), dtype=torch.int32 if k.endswith("_cells") else torch.float32,
                                     device=device) for k in ops._FLOW_ROWS} for _ in range(2)]
        carry = new(2, B, 3, Ho, Wo)                # the step's last predicted frame in physical units, for the next step's first pair
        before_score.append(lambda pred, step: ops.rollout_flow(pred, store.frames, first, step, store.out_tab, flow_channels, steps, float(flow.dx),
                                                                float(flow.dt), flow.band_width(), int(flow.interface_radius), carry, *flow_rows))
    hf_p = hf_t = None
    if heatflux is not None:
        hf_channels = heatflux.channels(fields)
        heatflux.check_width(Wo)
        heater = _to_device(heatflux.temperatures(plan.files, len(ds.traj_lens)), torch.float32, device)
        hf_p, hf_t = new(B, steps * T), new(B, steps * T)
        before_score.append(lambda pred, step: ops.rollout_heatflux(pred, store.frames, first, step, store.out_tab, *hf_channels, heater, steps, hf_p, hf_t,
                                                                    heatflux.x_min, heatflux.dx, heatflux.lc, heatflux.conductivity))
    bub = None
    if bubbles is not None:
        mb = int(bubbles.max_bubbles)
        rows = lambda *tail: [torch.empty((B, steps * T) + tail, dtype=torch.int32, device=device) for _ in range(2)]
        bub = {"count": rows(), "cells": rows(), "attached": rows(), "area": rows(mb)}
        bub_args = (bubbles.channel(fields), steps, int(bubbles.connectivity), mb, ops.bubble_census_workspace(2 * B * T, Ho, Wo, mb, device),
                    *bub["count"], *bub["cells"], *bub["attached"], *bub["area"])
        if not (bubbles.track or bubbles.match):
            before_score.append(lambda pred, step: ops.rollout_bubbles(pred, store.frames, first, step, store.out_tab, *bub_args))
        else:                                       # the labelled census in its place; its ring serves the links and the matches alike
            ring = torch.empty((2, 2, B, T, Ho, Wo), dtype=torch.int32, device=device)
            before_score.append(lambda pred, step: ops.rollout_bubbles_labelled(pred, store.frames, first, step, store.out_tab, *bub_args, ring))
        if bubbles.track:                           # the links of the pairs that end in this step
            link_rows = [{k: torch.empty((B,) + shape, dtype=torch.int32, device=device) for k, shape in ops._link_rows((steps * T - 1,), mb).items()}
                         for _ in range(2)]
            link_ws = ops.bubble_links_workspace(2 * B * T, mb, device)
            before_score.append(lambda pred, step: ops.rollout_bubble_links(pred, store.frames, first, step, store.out_tab, steps, mb, link_ws, ring,
                                                                            *bub["count"], *bub["attached"], *bub["area"], *link_rows))
        match_rows = None
        if bubbles.match:                           # every predicted frame of this step against the simulated one
            match_rows = {k: torch.empty(shape, dtype=dtype, device=device) for k, (shape, dtype) in ops._match_rows((B, steps * T), mb).items()}
            match_ws = ops.bubble_match_workspace(B * T, mb, device)
            before_score.append(lambda pred, step: ops.rollout_bubble_match(pred, store.frames, first, step, store.out_tab, steps, mb,
                                                                            float(bubbles.min_iou), match_ws, ring, *bub["count"], *bub["attached"],
                                                                            *bub["area"], match_rows))
    err_rows = None
    if errors is not None:
        err_sdf = fields.index(errors.sdf_field) if errors.sdf_field in fields else -1
        K = ops.shell_count(Ho, Wo)
        err_rows = {key: new(B, steps * T, C) for key in ("rmse", "max_error", "boundary_rmse")}
        if err_sdf >= 0:
            err_rows["interface_rmse"] = new(B, steps * T, C)
            err_rows["interface_cells"] = torch.empty((B, steps * T, C), dtype=torch.int32, device=device)
        if errors.spectra:
            err_rows["spectral_error"] = new(B, steps * T, C, 3)
            for key in ("spectrum_error", "spectrum_pred", "spectrum_target"):
                err_rows[key] = new(B, steps * T, C, K)
        err_ws = ops.field_errors_workspace(B * T * C, Ho, Wo, device)
        before_score.append(lambda pred, step: ops.rollout_errors(pred, store.frames, first, step, store.out_tab, err_sdf, steps, err_ws,
                                                                  int(errors.interface_radius), int(errors.bands[0]), int(errors.bands[1]),
                                                                  errors.spectra, **err_rows))

    ens_rows = None
    if members is not None:
        ens_rows = {key: new(Bt, steps * T, C) for key in ("mean_rmse", "spread", "crps")}
        if ensemble.rank_histogram:
            ens_rows["rank_hist"] = torch.empty((Bt, steps * T, C, members + 1), dtype=torch.int32, device=device)
        if ensemble.keep_mean:
            ens_rows["mean"] = new(Bt, steps * T, C, Ho, Wo)
        ens_ws = ops.ensemble_workspace(Bt * T * C, members, Ho, Wo, device)
        before_score.append(lambda pred, step: ops.rollout_ensemble(pred, store.frames, first, step, store.out_tab, steps, members, ens_ws,
                                                                    ensemble.fair, **ens_rows))

    def score(pred, step, next_in, arch):
        if pred.dtype != torch.float32 or not pred.is_contiguous():
            pred = pred.float().contiguous()
        if pred.shape != x.shape:
            raise ValueError(f"the model returned {tuple(pred.shape)} for an input of {tuple(x.shape)}: it cannot be fed back")
        for call in before_score:
            call(pred, step)
        ops.rollout_score(pred, store.frames, first, step, store.out_tab, sdf, steps, rel_l2, criterion, ws, eik_p, eik_t, next_in, arch)

    model.eval()
    with torch.no_grad():
        if use_graph:
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):           # warm-up as GraphedForward's, plus one scoring call on a throw-away counter (no copies)
                for _ in range(2):
                    out = model(x, *extra)
                score(out, torch.zeros(1, dtype=torch.int32, device=device), None, None)
            torch.cuda.current_stream().wait_stream(side)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                score(model(x, *extra), counter, x, archive)
            owner = model.__dict__.get("_bf_eval_owner")
            for _ in range(steps):
                if owner is not None:
                    ops.refresh_eval_weights(owner)         # a no-op while the parameters do not change
                graph.replay()
        else:
            for _ in range(steps):
                score(model(x, *extra), counter, x, archive)
    report = RolloutReport(rel_l2, criterion, eik_p, eik_t, plan.timesteps.to(device, non_blocking=True), fields, archive, hf_p, hf_t)
    if bub is not None:
        fraction = lambda cells: (cells.to(torch.float64) / float(Ho * Wo)).to(torch.float32)       # the quotient in fp64, rounded once
        report.bubble_count_pred, report.bubble_count_target = bub["count"]
        report.bubble_attached_pred, report.bubble_attached_target = bub["attached"]
        report.vapour_fraction_pred, report.vapour_fraction_target = (fraction(c) for c in bub["cells"])
        report.bubble_area_pred, report.bubble_area_target = bub["area"]
        report.bubble_dx = float(bubbles.dx)
        if bubbles.track:
            for key in ("events", "successor", "predecessor", "departure_area"):
                setattr(report, f"bubble_{key}_pred", link_rows[0][key])
                setattr(report, f"bubble_{key}_target", link_rows[1][key])
        if match_rows is not None:
            for key in ("match_pred", "match_target", "overlap", "displacement", "counts"):
                setattr(report, "bubble_match_" + key.replace("match_", ""), match_rows[key])
            report.bubble_mask_cells = match_rows["mask"]
    if err_rows is not None:
        for key, rows in err_rows.items():
            setattr(report, key, rows)
    if red_rows is not None:
        report.redistance_rounds, report.redistance_change = red_rows
    if flow_rows is not None:
        for name, member in _FLOW_ROW_NAMES.items():
            setattr(report, name + "_pred", flow_rows[0][member])
            setattr(report, name + "_target", flow_rows[1][member])
        report.flow_dx, report.flow_dt = float(flow.dx), float(flow.dt)
    if ens_rows is not None:
        report.ensemble_members = members
        for key, rows in ens_rows.items():
            setattr(report, "ensemble_" + key, rows)
    return report


FIELD_ROLES = ("dfun", "temperature", "velx", "vely")          # the fields plot_bubbleml draws, in its channel order


def render_rollouts(report: RolloutReport, data, starts: Sequence[int], save_dir, trajectories: Optional[Sequence[int]] = None, **kw) -> dict:
    """Pictures of a report made with ``evaluate_rollouts(..., keep_predictions=True)`` on the same ``data`` and ``starts``: for every chosen
    trajectory b (all by default) the simulated frames at ``report.timesteps[b]`` are gathered from the store as the scoring call reads them
    (``ops.clip_gather``) and ``plot_utils.plot_bubbleml`` writes ``save_dir/traj_<b>/plots/0000.png ...`` and ``relative_l2_error.csv``.
    Keyword arguments go to ``plot_bubbleml``; the channels follow the report's field names unless given.  Returns {b: its result}."""
    import os
    from .. import ops
    from .plot_utils import plot_bubbleml
    if report.predictions is None:
        raise ValueError("this report kept no predictions: call evaluate_rollouts(..., keep_predictions=True)")
    device = report.predictions.device
    store = _frames_store(data, device)
    B, frames, _, Ho, Wo = report.predictions.shape
    T = int(store.ds.time_window)
    plan = plan_rollouts(store.ds, starts, frames // T)
    if len(plan.first) != B or not torch.equal(plan.timesteps, report.timesteps.cpu()):
        raise ValueError("data and starts do not give the report's trajectories")
    kw.setdefault("channels", tuple(report.fields.index(n) if n in report.fields else -1 for n in FIELD_ROLES))
    chosen = list(range(B)) if trajectories is None else [int(b) for b in trajectories]
    out = {}
    for b in chosen:
        if not 0 <= b < B:
            raise IndexError(f"trajectory {b} is outside the report (0 .. {B - 1})")
        first = _to_device([plan.first[b]], torch.int64, device)
        targets = ops.clip_gather(store.frames, first, T, frames, store.out_tab, Ho, Wo)[0]      # the frames behind the first input clip
        out[b] = plot_bubbleml(report.predictions[b], targets, plan.timesteps[b], os.path.join(str(save_dir), f"traj_{b}"), **kw)
    return out
