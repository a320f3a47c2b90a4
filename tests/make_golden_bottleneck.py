"""TEST INFRASTRUCTURE ONLY -- generate tests/golden/bottleneck_*.npz by running the UNMODIFIED reference (oracle/ref_shim.py)
on the CPU in fp32 on seeded checkpoints and images (tests/bottleneck_reference.py: CASES).

Run where the reference tree exists:   python tests/make_golden_bottleneck.py

A fixture holds no weights and no program text: the contrast shift the checkpoint was made with (a calibration of the seeded
backbone, stored because it runs a backbone on the CPU), checksums of the regenerated images and weights, and the reference's
outputs -- its forward_all pyramids (levels 1..4 of both images, every s-th channel so that a level stays within 48 KB, with
the checksum of the whole level; level 4, the coarse stage's input, also whole), and per ksize corr4d, delta4d (packed code), the cal_coarse_matches rows and scores; for the
cases with regressors the predict_fine outputs."""
import contextlib
import io
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import bottleneck_reference as br  # noqa: E402
import golden_util as gu  # noqa: E402
from oracle import ref_shim  # noqa: E402
from patch2pix_amd.utils import synthetic  # noqa: E402


def reference_score_error(corr4d, delta4d, rows, scores, feats1, feats2, sd, k, upsample):
    """Largest distance of the reference's recorded scores from the scores of the fp64 evaluation of the same level-4 features
    (oracle/error_model.py), over the rows on which the two agree."""
    from oracle import error_model as em
    from oracle import p2p_oracle as orc
    model = em.ErrorModel(feats1[4][0], feats2[4][0], sd, ksize=k)
    planes = None if delta4d is None else tuple(d[0, 0] for d in delta4d)
    zrows, zscores = orc.cal_coarse_matches(model.Z, planes, k, upsample)
    same = (zrows == rows[0]).all(dim=1)
    return float((zscores[same] - scores[0][same].double()).abs().max())


def main():
    ref = ref_shim.load_reference()
    only = sys.argv[1:]                      # python tests/make_golden_bottleneck.py [--probe] [case ...]
    probe = "--probe" in only
    only = [a for a in only if a != "--probe"]
    for name, (backbone, cs, hw1, hw2, ksizes, reg, fi, seed, iseed) in br.CASES.items():
        if only and name not in only:
            continue
        ckpt = br.checkpoint(name, br.KAPPA)
        # the shift the calibration found: the difference between the plain and the shifted bias
        plain = synthetic.make_backbone_checkpoint(seed, backbone, cs, br.regressor_config(reg), fi)["state_dict"]
        key = next(k for k in plain if not torch.equal(plain[k], ckpt["state_dict"][k]))
        shift = plain[key] - ckpt["state_dict"][key]
        again = br.checkpoint(name, shift)["state_dict"]
        assert all(torch.equal(again[k], v) for k, v in ckpt["state_dict"].items()), "the stored shift does not reproduce the checkpoint"
        config = br.model_config(name, ckpt, torch.device("cpu"))
        with contextlib.redirect_stdout(io.StringIO()):
            net = ref.patch2pix.Patch2Pix(config)
        net.eval()
        im1, im2 = br.images(name)
        out = {"contrast_shift": shift.numpy(), "image_checksum": np.float64(gu.checksum([im1, im2])),
               "weights_checksum": np.float64(gu.checksum([v for v in ckpt["state_dict"].values() if v.is_floating_point()])),
               "upsample": np.int64(net.upsample)}
        with torch.no_grad():
            both = {}
            for tag, im in (("1", im1), ("2", im2)):
                feats = both[tag] = []
                net.extract.forward_all(im, feats, early_feat=True)
                for lv in range(1, 5):
                    smp, s = br.sample_channels(feats[lv][0])
                    out[f"pyr{tag}_l{lv}"], out[f"pyr{tag}_l{lv}_step"] = smp.numpy(), np.int64(s)
                    out[f"pyr{tag}_l{lv}_checksum"] = np.float64(gu.checksum([feats[lv]]))
                out[f"feat{tag}_l4"] = feats[4][0].numpy()           # the coarse stage's input, whole: sparse, it compresses
            for k in ksizes:
                corr4d, delta4d = net.forward(im1, im2, ksize=k)
                rows, scores = net.cal_coarse_matches(corr4d, delta4d, ksize=k, upsample=net.upsample, center=True)
                # A FIXTURE'S CONDITION (on the reference and fp64 alone): the recorded scores are within the 1e-5 bar of the exact
                # ones -- a fixture farther out would ask even an exact implementation for the reference's own rounding error.
                # A seed that misses it is replaced in br.CASES (--probe prints the figure without writing).
                err = reference_score_error(corr4d, delta4d, rows, scores, both["1"], both["2"], ckpt["state_dict"], k, int(net.upsample))
                print(f"{name} ksize {k} (checkpoint seed {seed}): reference scores {err:.2e} from fp64")
                assert probe or err <= br.SCORE_FIXTURE_BAR, f"{name}: choose another checkpoint seed"
                out[f"k{k}_corr4d"] = corr4d[0, 0].numpy()
                if delta4d is not None:
                    di, dj, dk, dl = [d[0, 0] for d in delta4d]
                    out[f"k{k}_delta"] = (((di * k + dj) * k + dk) * k + dl).to(torch.uint8).numpy()
                out[f"k{k}_rows"], out[f"k{k}_scores"] = rows[0].numpy().astype(np.int32), scores[0].numpy()
            if reg is not None:
                fine, fs, mid, ms, coarse = net.predict_fine(im1, im2, ksize=2, ncn_thres=0.0, mutual=True, return_all=True)
                out.update(fine=fine[0].numpy(), fine_scores=fs[0].numpy(), mid=mid[0].numpy(), mid_scores=ms[0].numpy(),
                           coarse=coarse[0].numpy().astype(np.int32))
        if probe:
            continue
        path = br.golden_path(name)
        np.savez_compressed(path, **out)
        print(f"{name}: {os.path.getsize(path)} bytes; upsample {int(net.upsample)}, "
              + ", ".join(f"k{k}: {out[f'k{k}_rows'].shape[0]} rows" for k in ksizes)
              + (f", {out['coarse'].shape[0]} proposals" if reg is not None else ""))


if __name__ == "__main__":
    main()
