"""Times the renderer on the GPU: ``render_panels`` for --frames frame pairs at --size x --size and --scale with HIP
events, beside a device-to-device copy of the same number of output bytes in the same run, and ``plot_bubbleml`` end to end (wall time and
its split into kernel, copy and compression) for --e2e-frames frames.  Prints one JSON line.

    python tools/render_bench.py --frames 3200 --size 192 --scale 2 --e2e-frames 320
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)


def clips(frames: int, size: int, device):
    """(pred, target) (frames, 4, size, size): the first sample trajectory tiled to size x size, its frames cycled; the prediction is the
    simulation one frame on, slightly scaled."""
    from bubbleformer_amd.data import hdf5_lite
    f = hdf5_lite.File(os.path.join(REPO, "tests", "golden", "samples", "sample_1.hdf5"))
    x = np.stack([np.asarray(f[k][...], dtype=np.float32) for k in ("dfun", "temperature", "velx", "vely")], axis=1)
    reps = -(-size // x.shape[-1])
    x = torch.from_numpy(np.tile(x, (1, 1, reps, reps))[:, :, :size, :size].copy()).to(device)
    idx = torch.arange(frames, device=device) % x.shape[0]
    return (x[(idx + 1) % x.shape[0]] * 0.97).contiguous(), x[idx].contiguous()


def timed(fn, repeats: int) -> float:
    """Median milliseconds of fn() by HIP events, after one warm-up call."""
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return float(np.median(out))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=3200)
    ap.add_argument("--size", type=int, default=192)
    ap.add_argument("--scale", type=int, default=2)
    ap.add_argument("--chunk", type=int, default=400, help="frames per launch")
    ap.add_argument("--e2e-frames", type=int, default=320)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--workers", type=int, default=8)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("render_bench needs the GPU: nothing is timed without one")
    from bubbleformer_amd.utils.plot_utils import RenderSpec, plot_bubbleml, render_panels
    dev = torch.device("cuda:0")
    spec = RenderSpec(scale=args.scale)
    ranges = [(-6.0, 2.0), (0.0, 1.0), (0.0, 6.0)]
    chunk = min(args.chunk, args.frames)
    pred, target = clips(chunk, args.size, dev)
    launches = -(-args.frames // chunk)
    image = render_panels(pred, target, ranges, spec)
    twin = torch.empty_like(image)
    per_launch = timed(lambda: render_panels(pred, target, ranges, spec), args.repeats)
    per_copy = timed(lambda: twin.copy_(image), args.repeats)
    out = {"frames": args.frames, "size": args.size, "scale": args.scale, "image": list(image.shape[1:]), "frames_per_launch": chunk,
           "output_bytes": int(image.numel()) * launches, "render_ms": per_launch * launches, "copy_ms": per_copy * launches,
           "render_over_copy": per_launch / per_copy, "render_us_per_frame": 1e3 * per_launch / chunk}
    del image, twin
    n = min(args.e2e_frames, chunk)
    with tempfile.TemporaryDirectory() as tmp:
        plot_bubbleml(pred[:2], target[:2], range(2), os.path.join(tmp, "warm"), spec=spec, workers=args.workers)
        t0 = time.perf_counter()
        res = plot_bubbleml(pred[:n], target[:n], range(n), tmp, spec=spec, workers=args.workers)
        wall = time.perf_counter() - t0
        size = sum(os.path.getsize(p) for p in res["files"])
    out["plot_bubbleml"] = {"frames": n, "workers": args.workers, "wall_s": wall, "ms_per_frame": 1e3 * wall / n, "png_bytes": size,
                            **{k + "_s": v for k, v in res["seconds"].items()}}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
