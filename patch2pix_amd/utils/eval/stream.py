"""Streaming form of `estimate_matches` for long pair lists (the "next" rows of SURVEY.md section 8f: image loading
and the backbone as producers of the hot path).

The reference matches one pair per call (utils/eval/model_helper.py:64-109): load and resize both images with PIL,
run the backbone twice, match, copy back.  For a stream of pairs (MegaDepth / HPatches style evaluation) the same
results can be produced much faster by
  * decoding / resizing images in a thread pool while the GPU works (PIL releases the GIL in its decoders),
  * running the backbone once on the 2*B images of B same-sized pairs,
  * keeping the whole batch on the device between the backbone and the result (Patch2Pix.predict_fine_device: coarse
    stage, filter_coarse, both regressors; ops.match_tail_batch: io_thres and scaling), one asynchronous copy of the
    match arrays per batch, three batches in flight -- the main thread only issues work;
  * (device_filter=False, or a network the device path does not cover) sharing one fine-stage launch between the B
    pairs and software-pipelining the host-side filter (Patch2Pix.coarse_async / fine_from_ticket).
`estimate_matches_stream` yields exactly the triples `estimate_matches` would return, in input order.
"""
from collections import deque
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from ...networks.resnet import pair_pyramids
from ... import staging
from ..datasets.preprocess import decode_pixels, load_im_pixels, normalise_pixels, resize_pixels_device, upload_pixels


class _Decoded:
    """A decoded image that is resized on the device: the original pixels, and as `shape` the [H,W,3] it will have (what
    batches are grouped by)."""
    __slots__ = ("pixels", "shape")

    def __init__(self, pixels, out_hw):
        self.pixels, self.shape = pixels, (out_hw[0], out_hw[1], 3)


def _load(job):
    idx, im1, im2, ksize, upsample, imsize = job[:6]
    if len(job) > 6 and job[6] == "device":                                   # decode only
        a1, hw1, s1 = decode_pixels(im1, ksize, upsample, imsize=imsize)
        a2, hw2, s2 = decode_pixels(im2, ksize, upsample, imsize=imsize)
        return idx, _Decoded(a1, hw1), _Decoded(a2, hw2), np.array([tuple(s1) + tuple(s2)]), job
    t1, s1 = load_im_pixels(im1, ksize, upsample, imsize=imsize)          # uint8 [H,W,3]: normalised on the device
    t2, s2 = load_im_pixels(im2, ksize, upsample, imsize=imsize)
    return idx, t1, t2, np.array([tuple(s1) + tuple(s2)]), job


_image_ring, _out_ring, _dev_ring = staging.PinnedRing(4), staging.PinnedRing(4), staging.PinnedRing(4)


def _upload(tensors, device):
    """Stack a list of equally shaped uint8 [H,W,3] images into a recycled PINNED batch buffer, start one asynchronous
    copy to the device and normalise there -> float32 [B,3,H,W].  (Stacking into pageable memory and copying from there cost 100-190 ms per batch of 8 pairs --
    more than the whole GPU work of the batch.)"""
    return normalise_pixels(staging.upload(tensors, device, _image_ring, stack=True))


def _upload_resize(first, second, device):
    """resize="device": the original pixels of both images of every pair in one pinned buffer and one copy, then one resize
    + normalise call per output size on the consuming stream -> (im1, im2, both); `both` is the [2B,3,H,W] tensor the two
    are halves of when the sizes agree (else None)."""
    pixels = upload_pixels([d.pixels for d in first + second], device)
    n = len(first)
    if first[0].shape == second[0].shape:
        both = resize_pixels_device(pixels, first[0].shape[:2], normalise=True)
        return both[:n], both[n:], both
    return (resize_pixels_device(pixels[:n], first[0].shape[:2], normalise=True),
            resize_pixels_device(pixels[n:], second[0].shape[:2], normalise=True), None)


def _staged(rec):
    """The host arrays of an issued batch, once its copy has run."""
    views = rec["staged"].wait()
    if views is None:
        raise RuntimeError("estimate_matches_stream: more batches in flight than staging slots")
    return [v.numpy() for v in views]


def _issue_fine(net, ticket, metas, ncn_thres, mutual):
    """filter_coarse on the host, the fine stage of the batch enqueued, its match arrays on their way to a pinned buffer:
    nothing here waits for the fine stage."""
    fine, conf, coarse = net.fine_from_ticket(ticket, ncn_thres=ncn_thres, mutual=mutual)
    counts = [f.shape[0] for f in fine]
    # one device-to-host copy for the whole batch: [fine x1,y1,x2,y2 | confidence | coarse x1,y1,x2,y2]
    packed = torch.cat([torch.cat(fine), torch.cat(conf)[:, None], torch.cat(coarse).float()], dim=1)
    return dict(staged=staging.readback([packed], _out_ring), counts=counts, metas=metas)


def _collect(rec, io_thres):
    packed, = _staged(rec)
    out, start = [], 0
    for n, to_original in zip(rec["counts"], rec["metas"]):
        rows = packed[start:start + n]
        start += n
        refined, confidence, proposals = rows[:, 0:4], rows[:, 4], rows[:, 5:9]
        keep = np.flatnonzero(confidence > io_thres)
        if keep.size:
            refined, confidence, proposals = refined[keep], confidence[keep], proposals[keep]
        out.append((to_original * refined, np.array(confidence, dtype=np.float32), to_original * proposals))
    return out


def _issue_device(net, f1, f2, group, ksize, ncn_thres, mutual, io_thres, epi=None):
    """Coarse stage, device-side filter_coarse, both regressors and the io_thres / scaling tail of the batch enqueued,
    the padded results on their way to pinned memory.  Nothing here waits for the GPU.  epi = (fundamentals, bins): the
    batch's epipolar distances and bin counts (two more launches on the tail's outputs) travel in the same slot."""
    from ... import ops
    fine, scores, coarse, counts = net.predict_fine_device(f1, f2, ksize=ksize, ncn_thres=ncn_thres, mutual=mutual)
    scale = np.concatenate([g[3] for g in group]).astype(np.float64)
    outs = ops.match_tail_batch(fine, scores, coarse, counts, scale, io_thres)
    if epi is not None:
        from .model_helper import epipolar_device
        outs = tuple(outs) + epipolar_device(outs[0], outs[2], outs[3], [epi[0][g[0]] for g in group], epi[1])
    return dict(staged=staging.readback(outs, _dev_ring), jobs=[g[4] for g in group], epi=epi)


def _collect_device(net, rec, ncn_thres, mutual, io_thres):
    m, s, c, n, *dists = _staged(rec)
    epi = rec.get("epi")
    if epi is not None:
        from .measure import EpipolarReport
        from .model_helper import epipolar_report
        fdist, fhist, cdist, chist = dists
    out = []
    for b, job in enumerate(rec["jobs"]):
        k = int(n[b])
        if k < 0:       # a coordinate outside the device filter's packed key (an image side >= 2^15): the per-pair host path
            from .model_helper import estimate_matches
            for f in (job[1], job[2]):      # file objects were read by the loader thread: rewind them for the second decode
                if hasattr(f, "seek"):
                    f.seek(0)
            item = estimate_matches(net, job[1], job[2], ksize=job[3], ncn_thres=ncn_thres, mutual=mutual, io_thres=io_thres,
                                    eval_type="fine", imsize=job[5])
            if epi is not None:
                item += (epipolar_report(item[0], item[2], epi[0][job[0]], epi[1]),)
            out.append(item)
        else:
            item = (m[b, :k].copy(), s[b, :k].copy(), c[b, :k].copy())
            if epi is not None:
                item += (EpipolarReport(fdist[b, :k].copy(), cdist[b, :k].copy(), fhist[b].astype(np.int64),
                                        chist[b].astype(np.int64), list(epi[1]), k),)
            out.append(item)
    return out


def _finish(net, ticket, metas, ncn_thres, mutual, io_thres):
    return _collect(_issue_fine(net, ticket, metas, ncn_thres, mutual), io_thres)


def _bounded_map(pool, fn, jobs, ahead):
    """pool.map with at most `ahead` items decoded but not yet consumed.  (Executor.map submits everything at once: the
    loader threads then run flat out, far ahead of the GPU, and every one of their Python-level steps competes with the
    main thread -- which issues a thousand launches per batch -- for the interpreter lock: measured 170 pairs/s with 16
    free-running loaders against 315 for the same stages run one after the other.)"""
    futures = deque()
    jobs = iter(jobs)
    for job in jobs:
        futures.append(pool.submit(fn, job))
        if len(futures) >= ahead:
            break
    while futures:
        item = futures.popleft().result()
        for job in jobs:
            futures.append(pool.submit(fn, job))
            break
        yield item


def estimate_matches_stream(net, pairs, ksize=2, ncn_thres=0.0, mutual=True, io_thres=0.25, imsize=None,
                            batch=8, workers=4, lookahead=None, device_filter=True, resize="host", fundamentals=None):
    """Generator over `pairs` (iterable of (im1, im2) paths / file objects): yields
    (matches float64 [M,4], scores float32 [M], coarse_matches float64 [M,4]) per pair, in order.
    workers: loader threads (a 480x640 JPEG pair decodes in 2 ms: a few threads feed the GPU); lookahead: pairs decoded
    ahead of the batch being matched (default 3 batches); device_filter=False keeps filter_coarse on the host (the
    reference's numpy semantics literally; same results, tests/test_gpu_parity.py); resize="device": the loader threads
    only decode, the bicubic resize (Pillow's, bit for bit: csrc/preprocess.hip) and the normalisation of a whole batch are
    one call on the device -- same results (tests/test_gpu_resize.py).
    fundamentals: a sequence of one [3,3] fundamental matrix per pair (x2^T F x1 = 0 in original-image pixels; `pairs` must
    then be a sequence as well) adds a fourth value to every item, the EpipolarReport estimate_matches_device(...,
    fundamental=F) returns, computed per batch on the device path (which it needs)."""
    if resize not in ("host", "device"):
        raise ValueError(f"resize must be 'host' or 'device', got {resize!r}")
    epi = None
    if fundamentals is not None:
        from ... import ops
        from .model_helper import check_fundamental
        pairs = list(pairs)
        if len(fundamentals) != len(pairs):
            raise ValueError(f"fundamentals holds {len(fundamentals)} matrices for {len(pairs)} pairs")
        epi = ([check_fundamental(F) for F in fundamentals], list(ops.EPI_BINS_EVAL))
    if resize == "device" and torch.device(net.device).type != "cuda":
        raise ValueError("resize='device' needs the network on a GPU")
    on_device = (device_filter and torch.device(net.device).type == "cuda" and getattr(net, "panc", 1) == 1
                 and hasattr(net, "predict_fine_device"))
    if epi is not None and not on_device:
        raise ValueError("fundamentals needs the device path (device_filter=True, a network on a GPU with panc 1)")
    jobs = ((i, a, b, ksize, net.upsample, imsize, resize) for i, (a, b) in enumerate(pairs))
    pending = deque()          # (ticket, metas) whose fine stage has not been issued yet
    issued = deque()           # batches whose fine stage is enqueued and whose results are being copied to the host
    with ThreadPoolExecutor(max_workers=max(1, workers)) as pool, torch.no_grad():
        loaded = _bounded_map(pool, _load, jobs, lookahead or 3 * batch)
        group = []

        def _take(rec):
            return _collect_device(net, rec, ncn_thres, mutual, io_thres) if "jobs" in rec else _collect(rec, io_thres)

        def flush():
            """Backbone on the 2*B images of the current group, coarse stage enqueued, ticket queued."""
            if not group:
                return
            both = None
            if resize == "device":
                im1, im2, both = _upload_resize([g[1] for g in group], [g[2] for g in group], net.device)
            else:
                im1 = _upload([g[1] for g in group], net.device)
                im2 = _upload([g[2] for g in group], net.device)
            f1, f2 = pair_pyramids(net.extract, im1, im2, both)
            if on_device:
                issued.append(_issue_device(net, f1, f2, group, ksize, ncn_thres, mutual, io_thres, epi))
            else:
                pending.append((net.coarse_async(f1, f2, ksize=ksize), [g[3] for g in group]))
            group.clear()

        for item in loaded:
            if group and (item[1].shape != group[0][1].shape or item[2].shape != group[0][2].shape or len(group) >= batch):
                flush()
                # three batches in flight: coarse stage of the newest enqueued before the previous one is filtered on the
                # host and its fine stage enqueued, before the results of the one before that are unpacked -- the main
                # thread waits for the GPU only when the GPU is what limits the stream
                while len(pending) > 1:
                    ticket, metas = pending.popleft()
                    issued.append(_issue_fine(net, ticket, metas, ncn_thres, mutual))
                while len(issued) > (2 if on_device else 1):
                    yield from _take(issued.popleft())
            group.append(item)
        flush()
        while pending:
            ticket, metas = pending.popleft()
            issued.append(_issue_fine(net, ticket, metas, ncn_thres, mutual))
        while issued:
            yield from _take(issued.popleft())
