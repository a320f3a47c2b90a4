"""TEST INFRASTRUCTURE shared by the resize tests: the case table, the image generator and a numpy restatement of
Pillow's 8-bit bicubic resampling (two separable passes, fixed-point coefficients with 22 fractional bits, int64
accumulation).  The restatement is proven against the installed Pillow in tests/test_resize_host.py; the installed
Pillow stays the yardstick of every other test."""
import math

import numpy as np

PRECISION_BITS = 22

# (in_h, in_w) -> (out_h, out_w)
CASES = [
    ((37, 53), (16, 32)),        # non-integer downscale on both axes
    ((131, 97), (16, 16)),       # ~8x and ~6x: long tap rows, bounds clipped at both borders
    ((12, 20), (32, 48)),        # upscale: filterscale clamps to 1, 5 taps
    ((48, 64), (48, 32)),        # horizontal pass only
    ((48, 64), (16, 64)),        # vertical pass only
    ((32, 32), (32, 32)),        # copy
    ((480, 640), (240, 320)),    # exact 2x
]
BIG_CASE = CASES[-1]             # too slow for the fiber emulator
MIXED_BATCH = ([(37, 53), (131, 97), (64, 64)], (32, 32))       # per-item sizes in one launch
CONTENTS = ["noise", "white", "black", "checker", "ramp"]


def case_id(case):
    (ih, iw), (oh, ow) = case
    return f"{ih}x{iw}-{oh}x{ow}"


def make_image(h, w, content, seed=0):
    """uint8 [h,w,3]."""
    if content == "noise":
        return np.random.default_rng(1000 * seed + 7 * h + w).integers(0, 256, (h, w, 3), dtype=np.uint8)
    if content == "white":
        return np.full((h, w, 3), 255, np.uint8)
    if content == "black":
        return np.zeros((h, w, 3), np.uint8)
    if content == "checker":         # 0/255 with period 3: bicubic overshoot reaches clip8 at both ends
        yy, xx = np.mgrid[0:h, 0:w]
        v = (((yy // 3) + (xx // 3)) % 2 * 255).astype(np.uint8)
        return np.repeat(v[:, :, None], 3, axis=2).copy()
    if content == "ramp":            # horizontal ramp, channels offset
        x = (np.arange(w) * 255 // max(w - 1, 1)).astype(np.int64)
        img = np.stack([x, 255 - x, (x * 2) % 256], axis=1)[None].repeat(h, axis=0)
        return img.astype(np.uint8)
    raise ValueError(content)


def pil_resize(img, out_hw):
    from PIL import Image
    return np.array(Image.fromarray(img, "RGB").resize((out_hw[1], out_hw[0]), Image.BICUBIC), dtype=np.uint8)


def _bicubic(x):
    a = -0.5
    if x < 0.0:
        x = -x
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def tables(in_size, out_size):
    """(bounds int32 [out,2] = (first input coordinate, taps), coefficients int32 [out,ksize]) -- a scalar port."""
    scale = in_size / out_size
    filterscale = max(scale, 1.0)
    support = 2.0 * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / filterscale
    bounds = np.zeros((out_size, 2), np.int32)
    coeffs = np.zeros((out_size, ksize), np.int32)
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        k = [_bicubic((x + xmin - center + 0.5) * ss) for x in range(xmax)]
        ww = 0.0
        for w in k:
            ww += w
        for x in range(xmax):
            v = k[x] / ww if ww != 0.0 else k[x]
            v *= float(1 << PRECISION_BITS)
            coeffs[xx, x] = int(-0.5 + v) if v < 0 else int(0.5 + v)
        bounds[xx] = (xmin, xmax)
    return bounds, coeffs


def _pass(img, bounds, coeffs):
    """Resample axis 1 of img [rows, n, 3] (uint8)."""
    src = img.astype(np.int64)
    out = np.empty((img.shape[0], bounds.shape[0], 3), np.uint8)
    for xx, (xmin, n) in enumerate(bounds):
        acc = (src[:, xmin:xmin + n, :] * coeffs[xx, :n].astype(np.int64)[None, :, None]).sum(axis=1) + (1 << (PRECISION_BITS - 1))
        out[:, xx, :] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return out


def resize(img, out_hw, tables_fn=tables):
    """The restatement: horizontal pass first, over the rows the vertical pass reads; a pass whose axis keeps its size is
    skipped; the intermediate image is uint8."""
    ih, iw = img.shape[:2]
    oh, ow = out_hw
    need_h, need_v = iw != ow, ih != oh
    if need_v:
        bv, cv = tables_fn(ih, oh)
        first, last = int(bv[0, 0]), int(bv[-1, 0] + bv[-1, 1])
    else:
        first, last = 0, ih
    cur = img
    if need_h:
        bh, ch = tables_fn(iw, ow)
        cur = _pass(cur[first:last], bh, ch)
    elif need_v:
        cur = cur[first:last]
    if need_v:
        bv = bv.copy()
        bv[:, 0] -= first
        cur = _pass(cur.transpose(1, 0, 2), bv, cv).transpose(1, 0, 2)
    return np.ascontiguousarray(cur)
