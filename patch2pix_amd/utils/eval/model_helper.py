"""Entry points of the matching path with the reference's names and contracts.

Role of reference utils/eval/model_helper.py: `load_model(ckpt_path, method, lprint)`,
`estimate_matches(net, im1, im2, ksize, ncn_thres, mutual, io_thres, eval_type, imsize)`,
`estimate_score(net, im1, im2, ksize, normalize, imsize)` (non-reference: the pair score of `cal_coarse_score`),
`refine_matches(im1_path, im2_path, net, coarse_matcher, io_thres, imsize, coarse_only)` and the two matcher
factories `init_patch2pix_matcher(args)` / `init_ncn_matcher(args)`.  Signatures, defaults and return layouts are the
reference's (what image-matching-toolbox binds to); the bodies are organised around the HIP library underneath.

Return contract of `estimate_matches` (reference :64-109):
    matches         float64 [M,4]  (x1, y1, x2, y2) in ORIGINAL image pixels
    scores          float32 [M]
    coarse_matches  float64 [M,4]  the coarse match each row was refined from (same as matches for eval_type='coarse')
"""
from argparse import Namespace
from concurrent.futures import ThreadPoolExecutor
from functools import partial

import numpy as np
import torch

from ..common.setup_helper import load_weights
from ..datasets.preprocess import (decode_pixels, load_im_flexible, load_im_pixels, load_im_tensor, normalise_pixels,
                                   resize_pixels_device, upload_pixels)
from ...networks.patch2pix import Patch2Pix
from ... import ops
from .measure import EpipolarReport

_SILENT = lambda *a, **k: None


# ------------------------------------------------------------------------------------------ model construction
def _base_config(device):
    """Inference configuration of reference :32-39 (change_stride on, proposals in chunks of 1200)."""
    return Namespace(device=device, training=False, backbone="ResNet34", change_stride=True, regr_batch=1200,
                     feat_idx=None, regressor_config=None, weights_dict=None)


def _configure_patch2pix(config, ckpt):
    """A full checkpoint (utils/train/helper.py:10-20) carries its own architecture description."""
    for field in ("backbone", "feat_idx", "regressor_config"):
        setattr(config, field, ckpt[field])
    config.weights_dict = ckpt["state_dict"]
    config.regressor_config.panc = 1          # evaluation never expands anchors (reference :46)


def _configure_ncn(config, ckpt):
    """NCNet-only checkpoints are a bare state_dict or {'state_dict': ...} (reference :53-57)."""
    config.weights_dict = ckpt["state_dict"] if isinstance(ckpt, dict) and "state_dict" in ckpt else ckpt


def load_model(ckpt_path, method="patch2pix", lprint=print):
    """Build the network on the current HIP device and load a reference-format checkpoint.
    `ckpt_path` may also be an already loaded checkpoint dict."""
    if not torch.cuda.is_available():
        raise RuntimeError("patch2pix_amd needs an MI355X (torch.cuda.is_available() is False); there is no CPU path")
    device = torch.device("cuda", torch.cuda.current_device())
    in_memory = isinstance(ckpt_path, dict)
    ckpt = ckpt_path if in_memory else load_weights(ckpt_path, device)
    config = _base_config(device)
    lprint("\nLoad model method:{} ".format(method))
    if "patch2pix" in method:
        _configure_patch2pix(config, ckpt)
        origin = "<in-memory checkpoint>" if in_memory else ckpt_path
        lprint(f"Ckpt:{origin} epochs:{ckpt['last_epoch'] + 1}" if "last_epoch" in ckpt else f"Ckpt:{origin}")
    elif "nc" in method:
        _configure_ncn(config, ckpt)
        lprint("Load pretrained weights: {}".format("<in-memory checkpoint>" if in_memory else ckpt_path))
    else:
        lprint("Wrong method name.")
    return Patch2Pix(config).eval()


def init_patch2pix_matcher(args):
    net = load_model(args.ckpt, method="patch2pix")
    return partial(_call_fine, net, args)


def init_ncn_matcher(args):
    net = load_model(args.ckpt, method="nc")
    return partial(_call_coarse, net, args)


def _call_fine(net, args, imq, imr):
    return estimate_matches(net, imq, imr, ksize=args.ksize, io_thres=args.io_thres, eval_type="fine", imsize=args.imsize)


def _call_coarse(net, args, imq, imr):
    return estimate_matches(net, imq, imr, ksize=args.ksize, ncn_thres=args.ncn_thres, eval_type="coarse",
                            imsize=args.imsize)


# ------------------------------------------------------------------------------------------ matching
# the second image of a pair is decoded while the first one is (PIL releases the GIL); the threads start with the first job
_decoders = ThreadPoolExecutor(max_workers=2, thread_name_prefix="p2p-decode")


def _decode_pair(decode, net, im1, im2, ksize, imsize):
    """`decode(im, ksize, upsample, imsize=)` of both images, the second one on the helper thread."""
    second = _decoders.submit(decode, im2, ksize, net.upsample, imsize=imsize)
    return decode(im1, ksize, net.upsample, imsize=imsize), second.result()


def _load_pair(net, im1, im2, ksize, imsize):
    """Both images as [1,3,H,W] tensors on the device + the (1,4) factors back to original pixels."""
    # PIL decode + bicubic resize on the host like the reference (load_im_flexible); the uint8 pixels go to the device and
    # are normalised there (bit-identical, a quarter of the upload)
    tensors, factors = [], ()
    for pixels, scale_wh in _decode_pair(load_im_pixels, net, im1, im2, ksize, imsize):
        tensors.append(normalise_pixels(pixels.unsqueeze(0).to(net.device)))
        factors += tuple(scale_wh)
    return tensors[0], tensors[1], np.array([factors])


def _load_pair_device(net, im1, im2, ksize, imsize):
    """`_load_pair` with only the decoding on the host: the original pixels of both images go up in one copy and are
    resized (Pillow's bicubic, bit for bit) and normalised on the device."""
    decoded = _decode_pair(decode_pixels, net, im1, im2, ksize, imsize)
    pixels = upload_pixels([d[0] for d in decoded], net.device)
    tensors = [resize_pixels_device(p, d[1], normalise=True) for p, d in zip(pixels, decoded)]
    return tensors[0], tensors[1], np.array([tuple(decoded[0][2]) + tuple(decoded[1][2])])


def _host(t):
    return t.detach().cpu().numpy()


def estimate_matches(net, im1, im2, ksize=2, ncn_thres=0.0, mutual=True, io_thres=0.25, eval_type="fine",
                     imsize=None):
    """Match one image pair (batch size 1, like the reference)."""
    t1, t2, to_original = _load_pair(net, im1, im2, ksize, imsize)

    if eval_type == "coarse":
        with torch.no_grad():
            rows, row_scores = net.predict_coarse(t1, t2, ksize=ksize, ncn_thres=ncn_thres, mutual=mutual)
        pixels = to_original * _host(rows[0])
        return pixels, _host(row_scores[0]), pixels

    if eval_type != "fine":
        raise ValueError(f"eval_type must be 'coarse' or 'fine', got {eval_type!r}")
    with torch.no_grad():
        refined, confidence, proposals = net.predict_fine(t1, t2, ksize=ksize, ncn_thres=ncn_thres, mutual=mutual)
    refined, confidence, proposals = _host(refined[0]), _host(confidence[0]), _host(proposals[0])

    # keep the confident matches; when none clears the threshold every match is returned (reference :97-105)
    confident = np.flatnonzero(confidence > io_thres)
    if confident.size:
        refined, confidence, proposals = refined[confident], confidence[confident], proposals[confident]
    return to_original * refined, confidence, to_original * proposals


def estimate_score(net, im1, im2, ksize=2, normalize="softmax", imsize=None):
    """The NCNet pair score of one image pair as a Python float (non-reference entry point; Patch2Pix.cal_coarse_score,
    reference networks/patch2pix.py:320-338, on the pair's consensus volume): images loaded like estimate_matches loads
    them (load_im_flexible), one coarse stage, no matches and no fine stage.  What a re-ranking loop calls per candidate."""
    ops.score_norm(normalize)
    t1, t2, _ = _load_pair(net, im1, im2, ksize, imsize)
    with torch.no_grad():
        return float(net.predict_score(t1, t2, ksize=ksize, normalize=normalize)[0])


def check_fundamental(F):
    """A fundamental matrix argument as a float64 [3,3] numpy array; ValueError for any other shape.  No GPU needed."""
    F = F.detach().cpu().numpy() if torch.is_tensor(F) else np.asarray(F)
    if F.shape != (3, 3):
        raise ValueError(f"a fundamental matrix must have shape [3,3], got {F.shape}")
    return F.astype(np.float64)


def epipolar_device(m, c, n, fundamentals, bins):
    """The Sampson distances and bin counts of the tail's device outputs (m, c [B,stride,4] float64, n int32 [B]) under the
    pairs' fundamental matrices [B,3,3] (host): one p2p_epipolar_batch call per list -> (fdist, fhist, cdist, chist) on the
    device.  Nothing here waits for the GPU."""
    Fd = ops.small_to_device(np.asarray(fundamentals, dtype=np.float64).reshape(-1, 3, 3), torch.float64, m.device)
    fdist, fhist = ops.epipolar_batch(m, n, Fd, kind="sampson", bins=bins)
    cdist, chist = ops.epipolar_batch(c, n, Fd, kind="sampson", bins=bins)
    return fdist, fhist, cdist, chist


def epipolar_report(matches, coarse, F, bins):
    """The EpipolarReport of rows that are on the host already (the pairs the device filter hands back to the host path):
    the same kernel on an upload of them."""
    k = len(matches)
    nb = len(bins) - 1
    if k == 0:
        return EpipolarReport(np.empty(0), np.empty(0), np.zeros(nb, np.int64), np.zeros(nb, np.int64), list(bins), 0)
    device = torch.device("cuda", torch.cuda.current_device())
    both = ops.small_to_device(np.stack([matches, coarse]).astype(np.float64), torch.float64, device)
    dist, hist = ops.epipolar_batch(both, None, np.stack([F, F]), kind="sampson", bins=bins)
    dist, hist = _host(dist), _host(hist).astype(np.int64)
    return EpipolarReport(dist[0], dist[1], hist[0], hist[1], list(bins), k)


def estimate_matches_device(net, im1, im2, ksize=2, ncn_thres=0.0, mutual=True, io_thres=0.25, imsize=None, resize="host",
                            fundamental=None, bins=None):
    """estimate_matches(eval_type='fine') with NOTHING between the image tensors and the result on the host
    (non-reference entry point): coarse stage, filter_coarse, both regressors and the io_thres / scaling tail of
    model_helper.py:92-109 all run on the device; one device-to-host copy at the end.  Same return triple.
    resize="device": the bicubic resize runs on the device as well (csrc/preprocess.hip, equal to Pillow's bit for bit); the
    host only decodes.
    fundamental: a [3,3] matrix F with x2^T F x1 = 0 in ORIGINAL-image pixels adds a fourth value, an EpipolarReport
    (utils/eval/measure.py): the Sampson distances of the kept fine and coarse rows and their counts over `bins` (default: the
    list of the reference's eval_epoch_immatch.py:85), computed on the tail's device outputs before the copy -- what
    eval_epoch_immatch.py:62-63,85-87 computes on the host."""
    if resize not in ("host", "device"):
        raise ValueError(f"resize must be 'host' or 'device', got {resize!r}")
    if fundamental is not None:
        fundamental = check_fundamental(fundamental)
        bins = list(ops.EPI_BINS_EVAL if bins is None else bins)
        ops.epi_edges(bins)
    t1, t2, to_original = (_load_pair_device if resize == "device" else _load_pair)(net, im1, im2, ksize, imsize)
    with torch.no_grad():
        fine, scores, coarse, counts = net.predict_fine_device(net.extract.pyramid(t1), net.extract.pyramid(t2), ksize=ksize,
                                                               ncn_thres=ncn_thres, mutual=mutual)
        m, s, c, n = ops.match_tail_batch(fine, scores, coarse, counts, to_original, io_thres)
        epi = epipolar_device(m, c, n, fundamental[None], bins) if fundamental is not None else None
    k = int(n[0])
    if k < 0:          # a coordinate outside the device filter's packed key: the reference path
        out = estimate_matches(net, im1, im2, ksize, ncn_thres, mutual, io_thres, "fine", imsize)
        return out if fundamental is None else out + (epipolar_report(out[0], out[2], fundamental, bins),)
    out = _host(m[0, :k]), _host(s[0, :k]), _host(c[0, :k])
    if fundamental is None:
        return out
    fdist, fhist, cdist, chist = epi
    return out + (EpipolarReport(_host(fdist[0, :k]), _host(cdist[0, :k]), _host(fhist[0]).astype(np.int64),
                                 _host(chist[0]).astype(np.int64), bins, k),)


def refine_matches(im1_path, im2_path, net, coarse_matcher, io_thres=0.0, imsize=None, coarse_only=False):
    """Refine the matches of a third-party coarse matcher (reference :111-127): `coarse_matcher(grey1, grey2)` gets
    the two grey images [1,1,H,W] and returns [N,4] pixel matches in the loaded images' frame."""
    im1, grey1, sc1 = load_im_tensor(im1_path, net.device, imsize, with_gray=True)
    im2, grey2, sc2 = load_im_tensor(im2_path, net.device, imsize, with_gray=True)
    to_original = np.array([sc1 + sc2])
    coarse = coarse_matcher(grey1, grey2)
    if coarse_only:
        return to_original * coarse.cpu().data.numpy(), None, None
    with torch.no_grad():
        refined, scores, coarse = net.refine_matches(im1, im2, coarse, io_thres)
    return to_original * refined, scores, to_original * coarse
