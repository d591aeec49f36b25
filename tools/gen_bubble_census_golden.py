"""Golden values for the bubble census, generated on the CPU with scipy (the GPU tests need no scipy: they compare with this file and with
the flood fill of tests/bubbles_restatement.py).

    python tools/gen_bubble_census_golden.py

writes tests/golden/bubble_census.npz (arrays only):
  * labels/<mask>/<connectivity>: `scipy.ndimage.label` of every synthetic mask of tests/bubbles_restatement.py at its 40 x 72, as int16;
  * sample<k>/{count,attached}/<connectivity> (frames,) and sample<k>/areas/<connectivity> (frames, widest count), zero-padded, in label order:
    the components of dfun > 0 of every frame of tests/golden/samples/sample_<k>.hdf5.
The tool asserts what the tests rely on: the restatement's flood fill gives scipy's label image (the same numbering, compared with ==) on
every mask and every sample frame for both connectivities, the masks have the component counts the restatement lists, and no dfun cell of
the samples is exactly 0 or NaN (so `> 0` and `>= 0` name the same mask there)."""
import os
import sys

import numpy as np
from scipy import ndimage

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden")
if REPO not in sys.path:
    sys.path.insert(0, REPO)

STRUCTURE = {4: ndimage.generate_binary_structure(2, 1), 8: ndimage.generate_binary_structure(2, 2)}


def scipy_label(mask, connectivity):
    lab, n = ndimage.label(mask, structure=STRUCTURE[connectivity])
    return lab.astype(np.int32), int(n)


def main():
    from bubbleformer_amd.data import hdf5_lite
    from tests import bubbles_restatement as R
    out = {}
    for name, mask in R.masks().items():
        for ci, conn in enumerate(R.CONNECTIVITIES):
            lab, n = scipy_label(mask, conn)
            mine, m = R.label(mask, conn)
            assert n == m == R.MASK_COUNTS[name][ci], (name, conn, n, m)
            assert np.array_equal(lab, mine), (name, conn)
            out[f"labels/{name}/{conn}"] = lab.astype(np.int16)
    for k in (1, 2):
        dfun = np.asarray(hdf5_lite.File(os.path.join(GOLDEN, "samples", f"sample_{k}.hdf5"))["dfun"][:])
        assert dfun.dtype == np.float32 and not np.any(dfun == 0) and not np.any(np.isnan(dfun))
        for conn in R.CONNECTIVITIES:
            counts, attached, areas = [], [], []
            for frame in dfun:
                lab, n = scipy_label(frame > 0, conn)
                assert np.array_equal(lab, R.label(frame > 0, conn)[0]), (k, conn)
                counts.append(n)
                attached.append(len(np.unique(lab[0][lab[0] > 0])))
                areas.append(np.bincount(lab.ravel(), minlength=n + 1)[1:])
            pad = np.zeros((len(areas), max(counts)), np.int32)
            for i, a in enumerate(areas):
                pad[i, :len(a)] = a
            out[f"sample{k}/count/{conn}"] = np.asarray(counts, np.int32)
            out[f"sample{k}/attached/{conn}"] = np.asarray(attached, np.int32)
            out[f"sample{k}/areas/{conn}"] = pad
            print(f"sample_{k}, connectivity {conn}: {min(counts)} .. {max(counts)} components per frame, {min(attached)} .. {max(attached)} on row 0")
    path = os.path.join(GOLDEN, "bubble_census.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
