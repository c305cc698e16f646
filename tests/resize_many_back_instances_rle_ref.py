"""COCO's uncompressed run-length encoding restated in numpy, shared by resize_many_back_instances_rle's CPU and GPU tests.  Not a test
module.  The masks it is fed on the GPU are those of resize_many_back_instances(mask_format="bool"); every comparison is equality."""
import numpy as np


def rle(mask: np.ndarray) -> list:
    """mask [oh, ow] bool -> counts: the run lengths of the column-major (y fastest) vector, zeros first."""
    v = np.concatenate([[0], np.asarray(mask, bool).T.ravel().astype(np.int8)])
    edges = np.flatnonzero(np.diff(v))  # the flat positions where a run starts (position 0: the mask starts set, counts[0] = 0)
    return np.diff(np.concatenate([[0], edges, [mask.size]])).tolist()


def rows(masks, max_runs: int):
    """masks [M, oh, ow] -> (runs [M, max_runs] int32: the first max_runs counts, zero-padded; nruns [M] int32: the true lengths)."""
    runs, nruns = np.zeros((len(masks), max_runs), np.int32), np.zeros(len(masks), np.int32)
    for m, mask in enumerate(masks):
        counts = rle(mask)
        nruns[m] = len(counts)
        runs[m, :min(len(counts), max_runs)] = counts[:max_runs]
    return runs, nruns
