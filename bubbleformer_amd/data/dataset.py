"""Clip supply for the training step.

``BubbleForecast`` keeps the reference class's constructor, ``__len__``, ``normalize`` and ``__getitem__`` contract
(bubbleformer/data/dataset.py:17-184) but reads the trajectory files with the in-tree HDF5 reader (no h5py), and adds the
MI355X-side path: ``device_store()`` puts every trajectory in HBM once (a BubbleML study is a few GB; one GPU has 288 GB) and
``DeviceClipStore.gather`` builds a whole batch of normalised (input, target) clips with ONE HIP kernel (`bf_clip_gather`,
csrc/clip_store.hip) -- no host-side slicing, stacking or H2D copy per step.  ``device_store(dev, storage="q16")`` holds the same
trajectories as 16-bit codes in half the bytes and decodes them inside that launch (``Q16ClipStore``, csrc/clip_store_q16.hip).
"""
import json
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch
from torch.utils.data import Dataset

from . import hdf5_lite

FLUID_PARAM_KEYS = ("inv_reynolds", "cpgas", "mugas", "rhogas", "thcogas", "stefan", "prandtl")       # dataset.py:165-178, then heater.*


def _fluid_vector(fp: dict) -> List[float]:
    return [fp[k] for k in FLUID_PARAM_KEYS] + [fp["heater"]["nucWaitTime"], fp["heater"]["wallTemp"]]


# (offset, scale) of one file's field from its {mean, std, min, max}; the dataset's constants are the means of these over the files
_NORMS = {
    "none": lambda st: (0.0, 1.0),
    "std": lambda st: (st["mean"], st["std"]),
    "minmax": lambda st: (st["min"], st["max"] - st["min"]),
    "tanh": lambda st: ((st["max"] + st["min"]) / 2.0, (st["max"] - st["min"]) / 2.0),
}


def _host_constants(x: Optional[np.ndarray], norm: str) -> Tuple[float, float]:
    if norm not in _NORMS:
        raise ValueError(f"Unknown normalization type: {norm}")
    if x is None:
        return _NORMS[norm]({})
    need = {"std": ("mean", "std"), "minmax": ("min", "max"), "tanh": ("min", "max")}[norm]
    return _NORMS[norm]({k: getattr(x, k)() for k in need})      # numpy's own reductions in the array's dtype, as the reference's h5py arrays give


def _combine_constants(per_file: Dict[str, List[Tuple[float, float]]]) -> Tuple[Dict, Dict]:
    diff = {f: np.mean([c[0] for c in cs]).item() for f, cs in per_file.items()}
    div = {f: np.mean([c[1] for c in cs]).item() + 1e-8 for f, cs in per_file.items()}
    return diff, div


class BubbleForecast(Dataset):
    """Dataset class for time series forecasting on the BubbleML dataset (reference: bubbleformer/data/dataset.py:17)."""

    def __init__(self, filenames: List[str], input_fields: Optional[List[str]] = None, output_fields: Optional[List[str]] = None,
                 norm: str = "none", downsample_factor: int = 1, time_window: int = 16, start_time: int = 50,
                 return_fluid_params: bool = False):
        super().__init__()
        self.filenames = filenames
        self.input_fields = input_fields if input_fields is not None else ["dfun", "temperature", "velx", "vely"]
        self.output_fields = output_fields if output_fields is not None else ["dfun", "temperature", "velx", "vely"]
        self.norm = norm
        self.downsample_factor = downsample_factor
        self.time_window = time_window
        self.start_time = start_time
        self.data = [hdf5_lite.File(filename, "r") for filename in filenames]
        self.num_trajs = [1 for _ in self.data]
        self.traj_lens = [f[self.input_fields[0]].shape[0] for f in self.data]
        self.input_num_fields = len(self.input_fields)
        self.output_num_fields = len(self.output_fields)
        self.fields = list(set(self.input_fields + self.output_fields))
        self.diff_terms = {k: [] for k in self.fields}
        self.div_terms = {k: [] for k in self.fields}
        self.return_fluid_params = return_fluid_params
        if self.return_fluid_params:
            self.fluid_params = []
            for fname in filenames:
                with open(fname.replace(".hdf5", ".json"), "r", encoding="utf-8") as f:
                    self.fluid_params.append(json.load(f))

    @classmethod
    def from_arrays(cls, trajectories: Sequence[Dict[str, np.ndarray]], fluid_params: Optional[Sequence[dict]] = None, **kw) -> "BubbleForecast":
        """The same dataset over trajectories that are already in memory: one dict {field: array [frames][H][W]} per simulation in
        place of one HDF5 file each (synthetic or pre-loaded studies; bench.py's clip-supply leg).  Keyword arguments as the constructor's."""
        self = cls([], **{k: v for k, v in kw.items() if k != "return_fluid_params"})
        self.data = [dict(t) for t in trajectories]
        self.num_trajs = [1 for _ in self.data]
        self.traj_lens = [t[self.input_fields[0]].shape[0] for t in self.data]
        self.return_fluid_params = fluid_params is not None
        if fluid_params is not None:
            if len(fluid_params) != len(self.data):
                raise ValueError("one fluid-parameter record per trajectory")
            self.fluid_params = list(fluid_params)
        return self

    # ---------------------------------------------------------------- reference contract
    def _per_traj(self) -> List[int]:
        return [n * (t - self.start_time - 2 * self.time_window + 1) for n, t in zip(self.num_trajs, self.traj_lens)]

    def __len__(self) -> int:
        return sum(self._per_traj())

    def normalize(self, diff_terms: Optional[Dict] = None, div_terms: Optional[Dict] = None) -> Tuple[Dict, Dict]:
        """Channel-wise normalisation constants (the reference's contract, dataset.py:73-117): per field, the mean over files of that file's
        (offset, scale) under ``self.norm``, with 1e-8 added to the scale; or the constants handed in (a validation set takes the training
        set's).  This is the HOST path (numpy over the whole field of every file, as the reference computes them): what a CPU-only caller and
        ``norm="none"`` use.  With the trajectories resident in HBM, ``device_store(...).normalize()`` gets the same constants from one
        reduction launch instead of a host pass over every file."""
        if diff_terms is None and div_terms is None:
            per_file = {f: [_host_constants(None if self.norm == "none" else h5[f][...], self.norm) for h5 in self.data] for f in self.fields}
            diff_terms, div_terms = _combine_constants(per_file)
        self.diff_terms = diff_terms
        self.div_terms = div_terms
        return self.diff_terms, self.div_terms

    def locate(self, idx: int) -> Tuple[int, int]:
        """Sample index -> (file index, first input frame) (dataset.py:120-128)."""
        cumulative = np.cumsum(self._per_traj())
        file_idx = int(np.searchsorted(cumulative, idx, side="right"))
        start = idx + self.start_time - (int(cumulative[file_idx - 1]) if file_idx > 0 else 0)
        return file_idx, int(start)

    def unrollable(self, k: int) -> List[int]:
        """Sample indices whose ``k`` consecutive target clips all lie in the sample's own file -- what a training step unrolled through
        ``k`` of its own predictions can be fed: of a file of ``n`` frames the first ``n - start_time - (k + 1) * time_window + 1`` samples
        (none when that is <= 0; utils.rollout.plan_rollouts counts the same way for evaluation).  ``k = 1`` is every sample."""
        if int(k) != k or k < 1:
            raise ValueError(f"unrollable: k {k!r} must be an integer >= 1")
        out, base = [], 0
        for per, n, t in zip(self._per_traj(), self.num_trajs, self.traj_lens):
            out.extend(range(base, base + max(0, min(per, n * (t - self.start_time - (int(k) + 1) * self.time_window + 1)))))
            base += per
        return out

    def _field_clip(self, file_idx: int, field: str, sl: slice) -> torch.Tensor:
        item = torch.from_numpy(np.array(self.data[file_idx][field][sl], dtype=np.float32))
        if self.downsample_factor > 1:
            _, h, w = item.shape
            item = torch.nn.functional.interpolate(item.unsqueeze(1), size=(h // self.downsample_factor, w // self.downsample_factor),
                                                   mode="nearest").squeeze(1)
        return (item - self.diff_terms[field]) / self.div_terms[field]

    def __getitem__(self, idx: int):
        file_idx, start = self.locate(idx)
        tw = self.time_window
        inp = torch.stack([self._field_clip(file_idx, f, slice(start, start + tw)) for f in self.input_fields])          # (C, T, H, W)
        out = torch.stack([self._field_clip(file_idx, f, slice(start + tw, start + 2 * tw)) for f in self.output_fields])
        if self.return_fluid_params:
            fp = torch.tensor(_fluid_vector(self.fluid_params[file_idx]), dtype=torch.float32)
            return inp.float().permute(1, 0, 2, 3), out.float().permute(1, 0, 2, 3), fp
        return inp.float().permute(1, 0, 2, 3), out.float().permute(1, 0, 2, 3)

    # ---------------------------------------------------------------- device-resident path
    def device_store(self, device, storage: str = "fp32", staging_frames: Optional[int] = None) -> "DeviceClipStore":
        """Every trajectory resident on ``device``.  ``storage="fp32"``: one fp32 tensor, filled through one host tensor of the dataset's size
        (``DeviceClipStore``).  ``storage="q16"``: 16-bit codes with one affine scale per (field, file), half the bytes, encoded on the device
        as the files are uploaded through two pinned staging buffers of ``staging_frames`` frames each (None: 64 MB's worth, at least 1) and
        decoded inside the gather's launch (``Q16ClipStore``; a GPU only: a CPU device raises ValueError)."""
        if storage == "fp32":
            return DeviceClipStore(self, device)
        if storage == "q16":
            return Q16ClipStore(self, device, staging_frames)
        raise ValueError(f"device_store: storage {storage!r} must be 'fp32' or 'q16'")


class DeviceClipStore:
    """Every trajectory of the dataset resident in HBM as one fp32 tensor ``[field][frame][H][W]`` (files concatenated along the
    frame axis); ``gather(indices)`` returns the batch the reference's DataLoader would have collated from ``dataset[i]``:
    ``(B, T, C_in, H', W')``, ``(B, T, C_out, H', W')`` [, ``(B, 9)`` fluid parameters] -- built by one kernel launch."""

    storage = "fp32"

    def __init__(self, ds: BubbleForecast, device, frames: Optional[torch.Tensor] = None):
        """``frames``: the resident tensor, when the caller has it already (``Q16ClipStore.to_fp32``); None reads the dataset's files."""
        self._setup(ds, device)
        if frames is None:
            total = int(self.frame0[-1])
            host = torch.empty((len(self.fields), total, self.H, self.W), dtype=torch.float32)
            for fi, f in enumerate(ds.data):
                for ci, name in enumerate(self.fields):
                    host[ci, self.frame0[fi]:self.frame0[fi + 1]] = torch.from_numpy(np.array(f[name][...], dtype=np.float32))
            frames = host.to(self.device)
        self.frames = frames
        self._tables()

    def _setup(self, ds: BubbleForecast, device):
        """Everything but the frames: the geometry, the field order, the files' places on the frame axis, the fluid rows."""
        self.ds = ds
        self.device = torch.empty(0, device=device).device      # indexed ("cuda" -> "cuda:0"): gather() compares index tensors' devices with it
        shapes = {tuple(f[ds.fields[0]].shape[1:]) for f in ds.data}
        if len(shapes) != 1:
            raise ValueError(f"device store needs one spatial resolution per dataset, got {sorted(shapes)}")
        (self.H, self.W), = shapes
        self.fields = sorted(ds.fields)
        self.frame0 = np.concatenate([[0], np.cumsum(ds.traj_lens)]).astype(np.int64)       # first frame of each file on the frame axis
        self._unroll_masks = {}       # per (dataset geometry, k): which samples are in ds.unrollable(k)
        self._odd_tabs = {}           # per (odd fields, input fields, output fields): the sign-eligibility tables of gather(augment=...)
        self.fluid = None
        if ds.return_fluid_params:
            self.fluid = torch.tensor([_fluid_vector(fp) for fp in ds.fluid_params], dtype=torch.float32, device=self.device)

    @property
    def nbytes(self) -> int:
        """Bytes the stored frames hold on the device."""
        return self.frames.numel() * self.frames.element_size()

    def normalize(self) -> Tuple[Dict, Dict]:
        """``BubbleForecast.normalize()`` from the trajectories in HBM: {sum, sum of squares, min, max} of every (field, file) segment by ONE
        reduction launch (bf_field_stats, fp64 accumulation in a fixed order) instead of a host pass over every file, then the reference's
        rule per file and the mean over files (dataset.py:84-117).  Sets the dataset's constants and this store's tables; returns them.
        Against the host path the constants agree to fp32 rounding of the host's own float32 reductions (~1e-7 relative)."""
        ds = self.ds
        if ds.norm == "none" or self.device.type != "cuda":
            out = ds.normalize()
            self._tables()
            return out
        if ds.norm not in _NORMS:
            raise ValueError(f"Unknown normalization type: {ds.norm}")
        st, n = self._segment_stats()
        nfile = len(ds.traj_lens)
        mean = st[..., 0] / n
        var = np.maximum(st[..., 1] / n - mean * mean, 0.0)
        per_file = {name: [_NORMS[ds.norm]({"mean": mean[ci, fi], "std": float(np.sqrt(var[ci, fi])), "min": st[ci, fi, 2], "max": st[ci, fi, 3]})
                           for fi in range(nfile)] for ci, name in enumerate(self.fields)}
        ds.diff_terms, ds.div_terms = _combine_constants(per_file)
        self._tables()
        return ds.diff_terms, ds.div_terms

    def _segment_stats(self) -> Tuple[np.ndarray, np.ndarray]:
        """{sum, sum of squares, min, max} in fp64 of every (field, file) segment of the resident frames, [fields][files][4], from ONE
        bf_field_stats launch, and the segments' element counts [fields][files]."""
        from .. import _lib as L
        from ..ops import _p, _stream
        ds = self.ds
        nfile, px = len(ds.traj_lens), self.H * self.W
        total = int(self.frame0[-1])
        begin = [(ci * total + int(self.frame0[fi])) * px for ci in range(len(self.fields)) for fi in range(nfile)]
        length = [int(ds.traj_lens[fi]) * px for _ in self.fields for fi in range(nfile)]
        nseg = len(begin)
        seg_b = torch.tensor(begin, dtype=torch.int64, device=self.device)
        seg_n = torch.tensor(length, dtype=torch.int64, device=self.device)
        out = torch.empty(nseg, 4, dtype=torch.float64, device=self.device)
        ws = torch.empty(L.lib().bf_field_stats_ws_doubles(nseg), dtype=torch.float64, device=self.device)
        L.check(L.lib().bf_field_stats(_p(self.frames), _p(seg_b), _p(seg_n), nseg, _p(out), _p(ws), _stream()), "bf_field_stats")
        st = out.cpu().view(len(self.fields), nfile, 4).numpy()
        n = np.asarray(length, dtype=np.float64).reshape(len(self.fields), nfile)
        return st, n

    def field_std(self) -> Dict[str, float]:
        """Per field, the standard deviation over ALL resident frames (every file pooled), in normalised units: the deviation of the stored
        values divided by the field's ``div`` constant (1 while the dataset has not been normalised) -- the scale ``NoiseSpec(relative=True)``
        refers to.  On the GPU from one bf_field_stats launch (sum and sum of squares per (field, file) segment in fp64, pooled on the host,
        as ``normalize()`` reads them); on a CPU store the same quantity from numpy in fp64."""
        ds = self.ds
        if self.device.type == "cuda":
            st, n = self._segment_stats()
            count = n.sum(axis=1)
            mean = st[..., 0].sum(axis=1) / count
            raw = np.sqrt(np.maximum(st[..., 1].sum(axis=1) / count - mean * mean, 0.0))
        else:
            raw = np.array([self.frames[ci].numpy().astype(np.float64).std() for ci in range(len(self.fields))])
        div = [1.0 if isinstance(ds.div_terms[name], list) else float(ds.div_terms[name]) for name in self.fields]
        return {name: float(raw[ci] / div[ci]) for ci, name in enumerate(self.fields)}

    def _tables(self):
        """Per-output-channel field index and normalisation constants; call again after ``ds.normalize()`` changed them."""
        ds = self.ds
        def tab(names):
            ids = torch.tensor([self.fields.index(n) for n in names], dtype=torch.int32, device=self.device)
            diff = torch.tensor([float(ds.diff_terms[n]) if not isinstance(ds.diff_terms[n], list) else 0.0 for n in names], dtype=torch.float32, device=self.device)
            div = torch.tensor([float(ds.div_terms[n]) if not isinstance(ds.div_terms[n], list) else 1.0 for n in names], dtype=torch.float32, device=self.device)
            return ids, diff, div
        self.in_tab, self.out_tab = tab(ds.input_fields), tab(ds.output_fields)

    def _index_tables(self):
        """Per sample index: absolute first input frame and file index, resident on the device (a few KB): gather() then needs no host
        work per step beyond the launch."""
        ds = self.ds
        key = (len(ds), ds.time_window, ds.start_time)
        if getattr(self, "_tab_key", None) != key:
            loc = [ds.locate(i) for i in range(len(ds))]
            self._first_all = torch.tensor([int(self.frame0[fi]) + st for fi, st in loc], dtype=torch.int64, device=self.device)
            self._file_all = torch.tensor([fi for fi, _ in loc], dtype=torch.int64, device=self.device)
            self._tab_key = key
        return self._first_all, self._file_all

    def _unrollable_mask(self, k: int) -> np.ndarray:
        """[len(ds)] bool: sample i is in ``ds.unrollable(k)`` (kept per k: the host-index check of gather(..., unroll=k))."""
        ds = self.ds
        key = (len(ds), ds.time_window, ds.start_time, int(k))
        cache = self._unroll_masks
        if key not in cache:
            mask = np.zeros(len(ds), dtype=bool)
            mask[np.asarray(ds.unrollable(k), dtype=np.int64)] = True
            cache[key] = mask
        return cache[key]

    def _odd_tables(self, odd_fields) -> Tuple[torch.Tensor, torch.Tensor]:
        """Per input / output channel, 1 where the channel's field is in ``odd_fields`` (int32 device tables; names the dataset lacks match nothing)."""
        ds = self.ds
        key = (tuple(odd_fields), tuple(ds.input_fields), tuple(ds.output_fields))
        cache = self._odd_tabs
        if key not in cache:
            cache[key] = tuple(torch.tensor([int(n in key[0]) for n in names], dtype=torch.int32, device=self.device) for names in key[1:])
        return cache[key]

    def gather(self, indices, unroll: Optional[int] = None, augment=None, draw: int = 0):
        """indices: sample indices as a sequence of ints or an integer tensor -- a DEVICE tensor (e.g. a slice of
        ``torch.randperm(len(ds), device=...)``) keeps the whole step free of host-device synchronisation; host indices are staged
        through pinned memory.
        ``unroll=k``: the batch of a training step unrolled through k of its own predictions, ``(inp, targets[, fluid])`` with ``targets``
        shaped ``(k, B, T, C_out, H', W')`` -- ``targets[j]`` contiguous, frames ``first + (j + 1) T .. first + (j + 2) T - 1`` -- still from
        one launch.  Host indices outside ``ds.unrollable(k)`` raise IndexError.  Device indices cannot be checked without a host
        synchronisation: they are clamped into the sample range, as without ``unroll``, and with ``unroll`` every frame number is also
        held below the store's frame count (bf_clip_gather_unroll; the single-clip launch needs no such clamp) -- a sample whose later
        clips lie behind its own file then yields the frames that follow on the store's frame axis, those of the next file, and the
        store's last frame where the store ends; so draw device indices from ``ds.unrollable(k)``.  ``unroll=None`` is the call it always was.
        ``augment``: a utils.augment.AugmentSpec -- per sample a seeded mirror in x (the odd fields change sign) and a seeded window of
        the output grid, decided on the device as a pure function of (spec.seed, sample index, ``draw``) and applied by the ONE launch
        that gathers (bf_clip_gather_augment): the clips come out ``(B, T, C, Hc, Wc)`` / ``(k, B, T, C, Hc, Wc)``, the fluid rows
        unchanged; ``utils.augment.augment_plan`` states the same decisions on the host.  A crop larger than the output grid and a CPU
        store raise ValueError.  None or an inactive spec: exactly the calls made without the argument, and ``draw`` is unread."""
        ds = self.ds
        if unroll is not None and (int(unroll) != unroll or unroll < 1):
            raise ValueError(f"gather: unroll {unroll!r} must be None or an integer >= 1")
        if augment is not None:
            from ..utils.augment import AugmentSpec
            if not isinstance(augment, AugmentSpec):
                raise ValueError(f"gather: augment {augment!r} must be None or a utils.augment.AugmentSpec")
            if not augment.active:
                augment = None
        if augment is not None:
            f = ds.downsample_factor
            window = augment.window(*((self.H // f, self.W // f) if f > 1 else (self.H, self.W)))
            if self.device.type != "cuda":
                raise ValueError("gather: augmentation runs inside the device gather (bf_clip_gather_augment); a CPU store has none")
        first_all, file_all = self._index_tables()
        if isinstance(indices, torch.Tensor) and indices.device == self.device:
            idx = indices.to(torch.int64)
        else:
            host = torch.as_tensor(np.asarray(indices, dtype=np.int64) if not isinstance(indices, torch.Tensor) else indices.to(torch.int64).cpu())
            if host.numel() and (int(host.min()) < 0 or int(host.max()) >= len(ds)):
                raise IndexError("sample index out of range")
            if unroll is not None and host.numel() and not bool(self._unrollable_mask(int(unroll))[host.numpy()].all()):
                raise IndexError(f"sample index outside unrollable({int(unroll)}): its target clips run past the end of its file")
            idx = host.pin_memory().to(self.device, non_blocking=True) if self.device.type == "cuda" else host.to(self.device)
        tw, f = ds.time_window, ds.downsample_factor
        ho, wo = (self.H // f, self.W // f) if f > 1 else (self.H, self.W)
        fl_files = file_all if self.fluid is not None else None
        inp, out, fl = self._launch(idx.contiguous(), first_all, fl_files, None if unroll is None else int(unroll), augment, window if augment is not None else None,
                                    int(draw), ho, wo)
        return (inp, out, fl) if self.fluid is not None else (inp, out)

    def _launch(self, idx, first_all, fl_files, unroll, augment, window, draw, ho, wo):
        """The gather's launch on this store's form -> (input clips, target clips, fluid rows or None)."""
        from .. import ops
        tw = self.ds.time_window
        if augment is not None:              # one launch: the mirrored / windowed input clip, target clips and the plain fluid rows
            from ..utils.augment import flip_threshold
            in_odd, out_odd = self._odd_tables(augment.odd_fields)
            inp, out, fl = ops.clip_gather_augment(self.frames, idx, first_all, tw, 1 if unroll is None else unroll, self.in_tab,
                                                   self.out_tab, ho, wo, in_odd, out_odd, augment.seed, draw, flip_threshold(augment.flip_p),
                                                   window[0], window[1], augment.crop_y == "random", augment.eval, self.fluid, fl_files)
            return inp, (out[0] if unroll is None else out), fl
        if unroll is not None:               # one launch: the input clip, all `unroll` target clips and the fluid rows
            return ops.clip_gather_unroll(self.frames, idx, first_all, tw, unroll, self.in_tab, self.out_tab, ho, wo, self.fluid, fl_files)
        if self.device.type == "cuda":       # one launch: both clips and the fluid rows, indexed by sample number on the device
            return ops.clip_gather_batch(self.frames, idx, first_all, tw, self.in_tab, self.out_tab, ho, wo, self.fluid, fl_files)
        first = first_all[idx]
        inp = ops.clip_gather(self.frames, first, 0, tw, self.in_tab, ho, wo)
        out = ops.clip_gather(self.frames, first, tw, tw, self.out_tab, ho, wo)
        return inp, out, (self.fluid[fl_files[idx]] if self.fluid is not None else None)


def q16_scale(lo, hi) -> Tuple[np.float32, np.float32]:
    """(step, inv) of a 16-bit segment whose values span lo .. hi (csrc/clip_store_q16.hip states the format): the quotients are taken in
    fp64 and rounded to fp32 once; a constant segment has both 0."""
    span = float(hi) - float(lo)
    if span == 0.0:
        return np.float32(0.0), np.float32(0.0)
    return np.float32(span / 65535.0), np.float32(65535.0 / span)


class Q16ClipStore(DeviceClipStore):
    """``DeviceClipStore`` in half the bytes: every value resident as a 16-bit code, one affine scale per (field, file) segment, decoded
    inside the gather's one launch (bf_clip_gather_q16; csrc/clip_store_q16.hip states the format, DESIGN.md section 27 the bound:
    ``|decoded - x| <= 0.53 step + 2^-24 max(|lo|, |hi|)``, step = (max - min) / 65535 of the segment).  A value closer to zero than half a
    step may come back with the other sign -- a ``dfun`` that close to the interface.  ``gather``, ``normalize``, ``field_std`` and the
    tables are DeviceClipStore's; ``gather`` returns bit for bit what ``to_fp32().gather`` returns.  There is no ``frames`` tensor: the
    rollout evaluation, which reads stored frames in its own kernels, takes ``to_fp32()``.

    The fill reads ONE field of ONE file on the host at a time, takes its minimum and maximum there, and sends it through two pinned
    buffers of ``staging_frames`` frames to two device buffers of that size, the copy of a chunk running beside the encode of the one
    before it: per chunk bf_field_stats on the staged fp32 values, then bf_clip_encode_q16 into the chunk's place.  Neither side ever
    holds the dataset in fp32.  The chunks' {sum, sum of squares, min, max} are combined on the host in fp64, in chunk order:
    ``normalize()`` and ``field_std()`` use these statistics of the ORIGINAL values, so the constants are the fp32 store's up to the order of
    an fp64 sum."""

    storage = "q16"
    STAGING_BYTES = 64 << 20

    def __init__(self, ds: BubbleForecast, device, staging_frames: Optional[int] = None):
        from .. import _lib as L
        from .. import ops
        from ..ops import _p, _stream
        if torch.empty(0, device=device).device.type != "cuda":
            raise ValueError("device_store: storage 'q16' is encoded and decoded by device kernels (csrc/clip_store_q16.hip); a CPU store has none")
        self._setup(ds, device)
        px, nfile, nfield, total = self.H * self.W, len(ds.traj_lens), len(self.fields), int(self.frame0[-1])
        sf = max(1, self.STAGING_BYTES // (px * 4)) if staging_frames is None else int(staging_frames)
        if sf < 1 or (staging_frames is not None and sf != staging_frames):
            raise ValueError(f"device_store: staging_frames {staging_frames!r} must be None or an integer >= 1")
        sf = min(sf, max(int(n) for n in ds.traj_lens))
        self.staging_frames = sf
        self.codes = torch.empty((nfield, total, self.H, self.W), dtype=torch.int16, device=self.device)      # the codes' bit patterns
        chunks = [[(a, min(a + sf, int(n))) for a in range(0, int(n), sf)] for n in ds.traj_lens]               # per file: its chunks' frame ranges
        lens = torch.tensor([(b - a) * px for _ in self.fields for file_chunks in chunks for a, b in file_chunks], dtype=torch.int64, device=self.device)
        zero = torch.zeros(1, dtype=torch.int64, device=self.device)
        stats = torch.empty((lens.numel(), 4), dtype=torch.float64, device=self.device)
        ws = torch.empty(L.lib().bf_field_stats_ws_doubles(1), dtype=torch.float64, device=self.device)
        pinned = [torch.empty((sf, self.H, self.W), dtype=torch.float32).pin_memory() for _ in range(2)]
        staged = [torch.empty((sf, self.H, self.W), dtype=torch.float32, device=self.device) for _ in range(2)]
        copied = [torch.cuda.Event() for _ in range(2)]       # the chunk in staged[b] has arrived (and pinned[b] may be refilled)
        encoded = [torch.cuda.Event() for _ in range(2)]      # staged[b] has been read (and may be overwritten)
        lo_tab, step_tab = np.zeros((nfield, nfile), dtype=np.float32), np.zeros((nfield, nfile), dtype=np.float32)
        with torch.cuda.device(self.device):
            main, side = torch.cuda.current_stream(), torch.cuda.Stream()
            k = 0
            for ci, name in enumerate(self.fields):
                for fi, f in enumerate(ds.data):
                    arr = np.array(f[name][...], dtype=np.float32)          # one field of one file: all the fp32 the host ever holds
                    lo, hi = arr.min(), arr.max()
                    step, inv = q16_scale(lo, hi)
                    lo_tab[ci, fi], step_tab[ci, fi] = lo, step
                    for a, b in chunks[fi]:
                        s = k & 1
                        if k >= 2:
                            copied[s].synchronize()
                        pinned[s][:b - a].copy_(torch.from_numpy(arr[a:b]))
                        with torch.cuda.stream(side):
                            if k >= 2:
                                side.wait_event(encoded[s])
                            staged[s][:b - a].copy_(pinned[s][:b - a], non_blocking=True)
                            copied[s].record(side)
                        main.wait_event(copied[s])
                        L.check(L.lib().bf_field_stats(_p(staged[s]), _p(zero), _p(lens) + 8 * k, 1, _p(stats) + 32 * k, _p(ws), _stream()), "bf_field_stats")
                        ops.clip_encode_q16(staged[s][:b - a], self.codes[ci, int(self.frame0[fi]) + a:int(self.frame0[fi]) + b], float(lo), float(inv))
                        encoded[s].record(main)
                        k += 1
            st = stats.cpu().numpy()                                         # waits for the last encode
            side.synchronize()
        del staged, pinned
        self._stats = np.zeros((nfield, nfile, 4), dtype=np.float64)
        k = 0
        for ci in range(nfield):
            for fi in range(nfile):
                acc = [0.0, 0.0, np.inf, -np.inf]
                for _ in chunks[fi]:
                    acc = [acc[0] + st[k, 0], acc[1] + st[k, 1], min(acc[2], st[k, 2]), max(acc[3], st[k, 3])]
                    k += 1
                self._stats[ci, fi] = acc
        self._counts = np.asarray([[int(n) * px for n in ds.traj_lens] for _ in self.fields], dtype=np.float64)
        self.frame_seg = torch.from_numpy(np.repeat(np.arange(nfile, dtype=np.int32), np.asarray(ds.traj_lens, dtype=np.int64))).to(self.device)
        self.seg_lo, self.seg_step = torch.from_numpy(lo_tab).to(self.device), torch.from_numpy(step_tab).to(self.device)
        self._tables()

    @property
    def nbytes(self) -> int:
        """Bytes the store holds on the device: the codes, the frames' file numbers and the two segment tables."""
        return sum(t.numel() * t.element_size() for t in (self.codes, self.frame_seg, self.seg_lo, self.seg_step))

    def _segment_stats(self) -> Tuple[np.ndarray, np.ndarray]:
        """The statistics taken while the store was filled -- those of the original values, not of the decoded ones."""
        return self._stats, self._counts

    def to_fp32(self) -> DeviceClipStore:
        """An ordinary ``DeviceClipStore`` over the decoded frames, filled by one decode launch: for small stores, rollout evaluation and tests."""
        from .. import ops
        return DeviceClipStore(self.ds, self.device, frames=ops.clip_decode_q16(self.codes, self.frame_seg, self.seg_lo, self.seg_step))

    def _launch(self, idx, first_all, fl_files, unroll, augment, window, draw, ho, wo):
        """One bf_clip_gather_q16 launch, whatever the call asks for."""
        from .. import ops
        aug = None
        if augment is not None:
            from ..utils.augment import flip_threshold
            aug = (*self._odd_tables(augment.odd_fields), augment.seed, draw, flip_threshold(augment.flip_p), window[0], window[1], augment.crop_y == "random",
                   augment.eval)
        inp, out, fl = ops.clip_gather_q16(self.codes, self.frame_seg, self.seg_lo, self.seg_step, idx, first_all, self.ds.time_window,
                                           1 if unroll is None else unroll, self.in_tab, self.out_tab, ho, wo, aug, self.fluid, fl_files)
        return inp, (out[0] if unroll is None else out), fl
