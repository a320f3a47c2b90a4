"""Image loading for matching -- role of reference utils/datasets/preprocess.py:32-60,83-91.

`load_im_tensor` (reference :7-30) is the loader of `refine_matches`: optional down-scaling to `imsize` with plain
rounding (no multiple-of-16 constraint), a grey copy for third-party coarse matchers, batch axis, on the device.
Host side (PIL) like the reference; the output feeds the backbone.  Target size = the original
size scaled so that max(w,h) == imsize (never up-sampled) and rounded *down* to a multiple of
upsample*k_size; bicubic resize; /255; ImageNet mean/std."""
import numpy as np
import torch
from PIL import Image

from ... import staging

_MEAN = np.array([0.485, 0.456, 0.406], dtype=np.float32).reshape(3, 1, 1)
_STD = np.array([0.229, 0.224, 0.225], dtype=np.float32).reshape(3, 1, 1)


def _normalised(img):
    arr = np.array(img, dtype=np.float32).transpose(2, 0, 1)
    arr /= 255.0
    return (torch.from_numpy(arr) - torch.from_numpy(_MEAN)) / torch.from_numpy(_STD)


_LUT = {}


def normalise_pixels(pixels):
    """uint8 [B,H,W,3] (any device) -> float32 [B,3,H,W], bit-identical to `_normalised`: the normalised value depends
    only on (channel, byte), so it is looked up in a [3,256] table computed ON THE HOST with the reference's three
    operations (/255, -mean, /std).  (The same arithmetic on the GPU is not bit-identical: its division by a constant is
    a multiplication by the reciprocal.)  Lets the entry points upload uint8 pixels -- a quarter of the bytes -- and
    skip the float conversion on the host."""
    dev = pixels.device
    if dev not in _LUT:
        v = np.arange(256, dtype=np.float32)[None, :].repeat(3, 0).reshape(3, 256, 1)
        v /= 255.0
        _LUT[dev] = ((torch.from_numpy(v) - torch.from_numpy(_MEAN)) / torch.from_numpy(_STD)).reshape(3, 256).to(dev)
    lut = _LUT[dev]
    idx = pixels.permute(0, 3, 1, 2).long()                                  # [B,3,H,W]
    return torch.gather(lut[None, :, :, None].expand(idx.shape[0], 3, 256, idx.shape[3]), 2, idx)


def load_im_pixels(im_path, k_size=2, upsample=16, imsize=None):
    """`load_im_flexible` up to (not including) the normalisation: -> (uint8 tensor [H,W,3], (wo/wt, ho/ht))."""
    img = Image.open(im_path).convert("RGB")
    wo, ho = img.width, img.height
    if not (imsize and imsize > 0) or imsize > max(wo, ho):
        imsize = max(wo, ho)
    wt, ht = cal_rescale_size(imsize, wo, ho, k_size=k_size, scale_factor=1.0 / upsample)
    img = img.resize((wt, ht), Image.BICUBIC)
    return torch.from_numpy(np.array(img, dtype=np.uint8)), (wo / wt, ho / ht)


def load_im_tensor(im_path, device, imsize=None, with_gray=True):
    """-> (im [1,3,H,W] normalised, gray [1,1,H,W] in [0,1], (wo/wt, ho/ht)) or (im, scale) without grey."""
    im = Image.open(im_path)
    wt, ht = wo, ho = im.width, im.height
    if imsize and max(wo, ho) > imsize and imsize > 0:
        s = imsize / max(wo, ho)
        ht, wt = int(round(ho * s)), int(round(wo * s))
        im = im.resize((wt, ht), Image.BICUBIC)
    scale = (wo / wt, ho / ht)
    gray = None
    if with_gray:
        g = np.array(im.convert("L"), dtype=np.float32) / 255.0
        gray = torch.from_numpy(g)[None, None].to(device)
    rgb = im if im.mode == "RGB" else im.convert("RGB")
    t = _normalised(rgb).unsqueeze(0).to(device)
    if with_gray:
        return t, gray, scale
    return t, scale


def cal_rescale_size(image_size, w, h, k_size=2, scale_factor=1 / 16, no_print=True):
    ratio = max(w, h) / image_size
    wt = int(np.floor(w / ratio * scale_factor / k_size) / scale_factor * k_size)
    ht = int(np.floor(h / ratio * scale_factor / k_size) / scale_factor * k_size)
    return wt, ht


def load_im_flexible(im_path, k_size=2, upsample=16, imsize=None, crop_square=False):
    img = Image.open(im_path).convert("RGB")
    wo, ho = img.width, img.height
    if not (imsize and imsize > 0) or imsize > max(wo, ho):
        imsize = max(wo, ho)
    wt, ht = cal_rescale_size(imsize, wo, ho, k_size=k_size, scale_factor=1.0 / upsample)
    img = img.resize((wt, ht), Image.BICUBIC)
    t = _normalised(img)
    if crop_square:
        t = t[:, :t.shape[2], :]
    return t, (wo / wt, ho / ht)


# ------------------------------------------------------------------------------------------ resize on the device
# Pillow's Image.resize(size, Image.BICUBIC) for 8-bit RGB is integer arithmetic on fixed-point coefficients, so the
# device kernels (csrc/preprocess.hip) reproduce it bit for bit.  The coefficients are computed HERE, on the host, in
# double precision with Pillow's operations in Pillow's order; the device only multiplies, adds, shifts and clamps.
_PRECISION_BITS = 22
_TABLES = {}


def resize_ksize(in_size, out_size):
    """Taps per output coordinate of the in_size -> out_size bicubic table (the row length of the coefficients)."""
    filterscale = max(in_size / out_size, 1.0)
    return int(np.ceil(2.0 * filterscale)) * 2 + 1


def resize_tables(in_size, out_size):
    """The table of one axis: (bounds int32 [out,2] = (first input coordinate, number of taps), coefficients int32
    [out, ksize] with 22 fractional bits, zero beyond a row's taps).  Cached per (in_size, out_size); read-only."""
    key = (int(in_size), int(out_size))
    if key in _TABLES:
        return _TABLES[key]
    in_size, out_size = key
    if in_size < 1 or out_size < 1:
        raise ValueError("resize_tables: sizes must be positive")
    scale = in_size / out_size
    filterscale = max(scale, 1.0)
    support = 2.0 * filterscale
    ksize = int(np.ceil(support)) * 2 + 1
    ss = 1.0 / filterscale
    center = (np.arange(out_size, dtype=np.float64) + 0.5) * scale
    xmin = np.maximum((center - support + 0.5).astype(np.int64), 0)          # C's (int) truncates; the values are > -1
    xmax = np.minimum((center + support + 0.5).astype(np.int64), in_size)
    count = xmax - xmin
    tap = np.arange(ksize, dtype=np.int64)[None, :]
    x = np.abs(((tap + xmin[:, None]) - center[:, None] + 0.5) * ss)
    w = np.where(x < 1.0, (1.5 * x - 2.5) * x * x + 1, np.where(x < 2.0, (((x - 5) * x + 8) * x - 4) * -0.5, 0.0))
    w = np.where(tap < count[:, None], w, 0.0)
    ww = np.add.accumulate(w, axis=1)[:, -1:]                                 # summed left to right, like the C loop
    w = np.where(ww != 0.0, w / np.where(ww != 0.0, ww, 1.0), w)
    w = w * float(1 << _PRECISION_BITS)
    coeffs = np.trunc(np.where(w < 0, -0.5 + w, 0.5 + w)).astype(np.int32)
    bounds = np.stack([xmin, count], axis=1).astype(np.int32)
    bounds.setflags(write=False)
    coeffs.setflags(write=False)
    _TABLES[key] = (bounds, coeffs)
    return _TABLES[key]


def _packed_table(in_size, out_size):
    """One axis as the int32 array the library reads: bounds [out,2] then coefficients [out,ksize]."""
    bounds, coeffs = resize_tables(in_size, out_size)
    return np.concatenate([bounds.reshape(-1), coeffs.reshape(-1)])


def _device_lut(dev):
    if dev not in _LUT:
        normalise_pixels(torch.zeros((1, 1, 1, 3), dtype=torch.uint8, device=dev))
    return _LUT[dev]


def resize_pixels_device(pixels, out_hw, normalise=False, out=None):
    """Pillow's bicubic resize of uint8 RGB images on the device, bit for bit: `pixels` is one uint8 [H,W,3] tensor or a
    list of them (any sizes) on one GPU; -> uint8 [B,Hout,Wout,3], or with normalise=True float32 [B,3,Hout,Wout] equal to
    `_normalised` of Pillow's result.  `out` (normalise=True only): a contiguous float32 [B,3,Hout,Wout] tensor -- e.g. a
    slice along the batch axis of a larger one -- that receives the result instead of a new tensor."""
    from ... import _lib, ops
    items = [pixels] if torch.is_tensor(pixels) else list(pixels)
    ho, wo = int(out_hw[0]), int(out_hw[1])
    if not items:
        raise ValueError("resize_pixels_device: no image")
    dev = items[0].device
    for t in items:
        if t.dtype != torch.uint8 or t.dim() != 3 or t.shape[2] != 3 or not t.is_cuda or t.device != dev:
            raise TypeError("resize_pixels_device: uint8 [H,W,3] tensors on one GPU expected")
    items = [t.contiguous() for t in items]
    nb = len(items)
    # one int32 array with every distinct axis table of the batch, uploaded through the pinned ring
    offsets, parts, at = {}, [], 0
    for t in items:
        for key in ((t.shape[1], wo), (t.shape[0], ho)):
            if key[0] != key[1] and key not in offsets:
                part = _packed_table(*key)
                offsets[key] = at
                parts.append(part)
                at += part.size
    tables = ops.small_to_device(np.concatenate(parts), torch.int32, dev) if parts else None
    desc = (_lib.ResizeItem * nb)()
    for i, t in enumerate(items):
        h, w = t.shape[0], t.shape[1]
        desc[i].pixels, desc[i].in_h, desc[i].in_w = t.data_ptr(), h, w
        if w != wo:
            desc[i].table_x, desc[i].ksize_x = tables.data_ptr() + 4 * offsets[(w, wo)], resize_ksize(w, wo)
        if h != ho:
            desc[i].table_y, desc[i].ksize_y = tables.data_ptr() + 4 * offsets[(h, ho)], resize_ksize(h, ho)
    if normalise:
        if out is None:
            out = torch.empty((nb, 3, ho, wo), dtype=torch.float32, device=dev)
        elif (tuple(out.shape) != (nb, 3, ho, wo) or out.dtype != torch.float32 or not out.is_contiguous()
              or out.device != dev):
            raise ValueError(f"out must be a contiguous float32 tensor of shape {(nb, 3, ho, wo)} on {dev}")
        lut = _device_lut(dev)
    else:
        if out is not None:
            raise ValueError("out is only for normalise=True")
        out = torch.empty((nb, ho, wo, 3), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        need = _lib.p2p_resize_workspace_bytes(nb, max(t.shape[0] for t in items), max(t.shape[1] for t in items), ho, wo)
        ws = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)        # stream-ordered by the allocator
        _lib.check(_lib.p2p_resize_bicubic_batch(desc, nb, ho, wo, None if normalise else out.data_ptr(),
                                                 out.data_ptr() if normalise else None, 3 * ho * wo,
                                                 lut.data_ptr() if normalise else None, ws.data_ptr(), need,
                                                 ops._stream()), "p2p_resize_bicubic_batch")
    return out


_decode_ring = staging.PinnedRing(4)


def upload_pixels(arrays, device):
    """uint8 [H,W,3] numpy arrays of any sizes -> device tensors, through ONE recycled pinned buffer and one
    asynchronous copy (staging.py; a copy from pageable memory would make the host wait for the stream)."""
    return staging.upload(arrays, device, _decode_ring)


def decode_pixels(im_path, k_size=2, upsample=16, imsize=None):
    """`load_im_pixels` without the resize: -> (uint8 array [ho,wo,3] of the ORIGINAL pixels, (ht, wt), (wo/wt, ho/ht))."""
    img = Image.open(im_path).convert("RGB")
    wo, ho = img.width, img.height
    if not (imsize and imsize > 0) or imsize > max(wo, ho):
        imsize = max(wo, ho)
    wt, ht = cal_rescale_size(imsize, wo, ho, k_size=k_size, scale_factor=1.0 / upsample)
    return np.asarray(img, dtype=np.uint8), (ht, wt), (wo / wt, ho / ht)


def load_im_flexible_device(im_path, device, k_size=2, upsample=16, imsize=None):
    """`load_im_flexible` with the resize and the normalisation on the device: decoded on the host, the original pixels
    uploaded through a recycled pinned buffer.  -> (float32 [3,H,W] on `device`, (wo/wt, ho/ht)), the same values."""
    arr, out_hw, scale = decode_pixels(im_path, k_size, upsample, imsize)
    pixels = upload_pixels([arr], device)
    return resize_pixels_device(pixels, out_hw, normalise=True)[0], scale
