"""Epipolar evaluation of matches with the reference's names -- role of reference utils/eval/measure.py:6-71,115-141:
`expand_homo_ones`, `sampson_distance`, `symmetric_epipolar_distance` and `check_inliers_distr`.

The distances and the bin counts come from one kernel (csrc/epipolar.hip, p2p_epipolar_batch): fp64 in a documented order
(include/p2p_hip.h).  Device tensors in -> a float64 device tensor out; numpy arrays in -> a float64 numpy array out, through
the same kernel on the current HIP device: the package has no CPU arithmetic path and this module adds none.  What stays on the
host is what the reference has there and what is no arithmetic on match rows: the mean over pairs and the formatting of
`check_inliers_distr`, in fp64.

Not here: the pose functions (`eval_matches_relapose`, `cal_vec_angle_error`, `cal_quat_angle_error`, `cal_rot_angle_error`) and
`eval_immatch_val_sets` of the reference's evaluation scripts.  They need OpenCV, transforms3d and COLMAP data, none of which
this package depends on; they are out of scope and have no stubs.
"""
from collections import namedtuple

import numpy as np
import torch

from ... import ops

# What estimate_matches_device(..., fundamental=F) and estimate_matches_stream(..., fundamentals=...) add to a pair's result:
# the Sampson distances of the kept fine and coarse rows in original-image pixels (float64 numpy [n]), their bin counts (int64
# numpy [len(bins) - 1]), the edges and the number of rows.
EpipolarReport = namedtuple("EpipolarReport", "fdist cdist fhist chist bins n")

DEFAULT_BINS = list(ops.EPI_BINS_MEASURE)


def expand_homo_ones(arr2d, axis=1):
    """Raise a 2D array, (N, 2) or (2, N), to homogeneous coordinates: ones appended along `axis` (measure.py:6-16)."""
    if axis == 0:
        ones = np.ones((1, arr2d.shape[1]))
    else:
        ones = np.ones((arr2d.shape[0], 1))
    return np.concatenate([arr2d, ones], axis=axis)


def _rows(pts1, pts2, homos):
    """Two point sets ([N,2] each; [N,3] with a third coordinate of 1 when homos is False) checked and cut to [N,2], and
    whether the caller gave numpy."""
    as_numpy = not torch.is_tensor(pts1)
    if as_numpy != (not torch.is_tensor(pts2)):
        raise ValueError("pts1 and pts2 must both be numpy arrays or both be tensors")
    if as_numpy:
        pts1, pts2 = np.asarray(pts1, dtype=np.float64), np.asarray(pts2, dtype=np.float64)
    width = 2 if homos else 3
    for name, p in (("pts1", pts1), ("pts2", pts2)):
        if p.ndim != 2 or p.shape[1] != width:
            raise ValueError(f"{name} must have shape (num_points, {width}) with homos={bool(homos)}, got {tuple(p.shape)}")
    if pts1.shape[0] != pts2.shape[0]:
        raise ValueError(f"pts1 and pts2 hold {pts1.shape[0]} and {pts2.shape[0]} points")
    if not homos:
        for p in (pts1, pts2):
            if not bool((p[:, 2] == 1).all()):
                raise NotImplementedError("homos=False with a third coordinate other than 1: the kernel works on (x, y, 1)")
        pts1, pts2 = pts1[:, :2], pts2[:, :2]
    return pts1, pts2, as_numpy


def _distance(pts1, pts2, F, homos, kind, eps):
    pts1, pts2, as_numpy = _rows(pts1, pts2, homos)
    if tuple(np.shape(F)) != (3, 3):
        raise ValueError(f"F must be a 3x3 matrix, got shape {tuple(np.shape(F))}")
    if pts1.shape[0] == 0:
        return np.empty((0,), dtype=np.float64) if as_numpy else torch.empty((0,), dtype=torch.float64, device=pts1.device)
    if as_numpy:
        if not torch.cuda.is_available():
            raise RuntimeError("patch2pix_amd needs an MI355X (torch.cuda.is_available() is False); there is no CPU path")
        device = torch.device("cuda", torch.cuda.current_device())
        rows = ops.small_to_device(np.concatenate([pts1, pts2], axis=1)[None], torch.float64, device)
    else:
        rows = torch.cat([pts1.to(torch.float64), pts2.to(device=pts1.device, dtype=torch.float64)], dim=1)[None]
    dist, _ = ops.epipolar_batch(rows, None, F if torch.is_tensor(F) else np.asarray(F, dtype=np.float64), kind=kind, eps=eps)
    return dist[0].cpu().numpy() if as_numpy else dist[0]


def sampson_distance(pts1, pts2, F, homos=True, eps=1e-8):
    """Sampson distance dd^2 / (eps + l1_0^2 + l1_1^2 + l2_0^2 + l2_1^2) between two sets of points (measure.py:18-40):
    pts1, pts2 (num_points, 2), F with x2^T F x1 = 0 -> (num_points,) float64."""
    return _distance(pts1, pts2, F, homos, "sampson", eps)


def symmetric_epipolar_distance(pts1, pts2, F, homos=True, sqrt=False):
    """Symmetric epipolar distance (measure.py:43-71; no eps, so a degenerate line divides by zero as in numpy): sqrt=False
    the squared form of Hartley & Zisserman, sqrt=True |dd| (1 / |l1| + 1 / |l2|)."""
    return _distance(pts1, pts2, F, homos, "sym_sqrt" if sqrt else "sym", 0.0)


def _histograms(dists, edges):
    """Bin counts of a list of non-empty one-dimensional arrays / tensors of distances: one launch for all of them."""
    nmax = max(len(d) for d in dists)
    rows = np.zeros((len(dists), nmax, 4), dtype=np.float64)
    for b, d in enumerate(dists):
        rows[b, :len(d), 0] = d.detach().cpu().numpy() if torch.is_tensor(d) else np.asarray(d, dtype=np.float64)
    if not torch.cuda.is_available():
        raise RuntimeError("patch2pix_amd needs an MI355X (torch.cuda.is_available() is False); there is no CPU path")
    device = torch.device("cuda", torch.cuda.current_device())
    rows_d, counts = ops.small_to_device(rows, torch.float64, device), ops.small_to_device(
        np.array([len(d) for d in dists], dtype=np.int32), torch.int32, device)
    out = []
    for b0 in range(0, len(dists), 65535):
        _, hist = ops.epipolar_batch(rows_d[b0:b0 + 65535], counts[b0:b0 + 65535], np.zeros((len(rows_d[b0:b0 + 65535]), 3, 3)),
                                     kind="value", bins=edges)
        out.append(hist.cpu().numpy().astype(np.int64))
    return np.concatenate(out)


def format_inliers_distr(hists, npts, nsamples, bins, tag="", return_ratios=False):
    """The string (and ratios) of check_inliers_distr from per-pair bin counts [P, nbins] and row counts [P] of the non-empty
    pairs; nsamples: the length of the list including the empty ones (measure.py:132-141, character for character)."""
    npts = np.asarray(npts)
    inlier_ratios = [np.asarray(h) / n for h, n in zip(hists, npts)]
    ratio_print = '{} Sample:{} N(mean/max/min):{:.0f}/{:.0f}/{:.0f}\nRatios(%):'.format(tag, nsamples, np.mean(npts), np.max(npts),
                                                                                        np.min(npts))
    ratios = []
    for val, low, high in zip(np.mean(inlier_ratios, axis=0), bins[0:-1], bins[1::]):
        ratio_print = '{} [{},{})={:.2f}'.format(ratio_print, low, high, 100 * val)
        ratios.append(100 * val)
    if return_ratios:
        return ratios, ratio_print
    return ratio_print


def check_inliers_distr(inlier_dists, bins=[0, 1e-2, 1, 5, 10, 25, 50, 100, 400, 2500, 1e5], tag='', return_ratios=False,
                        field=None):
    """The distribution of per-pair distances over `bins` as the reference prints it (measure.py:115-141): the same string,
    character for character, and with return_ratios the same ratios.  inlier_dists: a list of per-pair arrays / tensors of
    distances, or a list of EpipolarReport (then `field` picks 'fdist' or 'cdist'; default: 'cdist' when tag is 'cdist', else
    'fdist').  The bin counts are the kernel's (a report's own counts when it was made with these bins); the mean over pairs and
    the formatting are host fp64."""
    if not inlier_dists:
        if return_ratios:
            return None, ''
        return ''
    edges = ops.epi_edges(bins)
    if all(isinstance(d, EpipolarReport) for d in inlier_dists):
        field = field or ("cdist" if tag == "cdist" else "fdist")
        if field not in ("fdist", "cdist"):
            raise ValueError(f"field must be 'fdist' or 'cdist', got {field!r}")
        kept = [r for r in inlier_dists if r.n > 0]
        stored = all(len(r.bins) == len(edges) and np.array_equal(np.asarray(r.bins, dtype=np.float64), edges) for r in kept)
        dists = [getattr(r, field) for r in kept]
        hists = [getattr(r, "fhist" if field == "fdist" else "chist") for r in kept] if stored else None
    else:
        dists = [d for d in inlier_dists if len(d) > 0]
        hists = None
    if not dists:          # the reference takes the mean of an empty list here; say what is wrong instead
        raise ValueError("check_inliers_distr: every pair is empty")
    if hists is None:
        hists = _histograms(dists, edges)
    return format_inliers_distr(hists, [len(d) for d in dists], len(inlier_dists), list(bins), tag, return_ratios)
