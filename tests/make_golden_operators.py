"""TEST INFRASTRUCTURE ONLY -- generate the fixtures tests/golden/operators_<family>.npz by running the UNMODIFIED reference's
operators (networks/modules.py, networks/ncn/model.py, conv4d.py, extract_ncmatches.py) on the CPU over the cases of
tests/operators_reference.py, and measure the reference's own fp32 error against the float64 restatements.

Run where the reference tree exists:   python tests/make_golden_operators.py
A fixture holds the inputs and the reference's fp32 outputs (the 256-channel correlation case: the output alone, its inputs
come from the seed, and the fixture records their sha256).  The REF_ERR table it prints goes into tests/operators_reference.py.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle import ref_shim                          # noqa: E402
import operators_reference as orf                    # noqa: E402


def save(family, arrays):
    np.savez_compressed(orf.golden_name(family), **arrays)
    print(f"{orf.golden_name(family)}: {os.path.getsize(orf.golden_name(family))} bytes")


def main():
    ref = ref_shim.load_reference()
    table = {}
    with torch.no_grad():
        arrays = {}
        for case in orf.CORR_CASES:
            fa, fb = orf.corr_inputs(case)
            out = ref.modules.FeatCorrelation(shape='4D')(fa, fb)
            b = fa.shape[0]
            flat = out.reshape(b, fa.shape[2] * fa.shape[3], -1).contiguous()
            table[f"corr_{case}"] = orf.rel_err(flat, orf.correlation64(fa, fb))
            if case != "B":
                arrays[f"a_{case}"], arrays[f"b_{case}"] = fa.numpy(), fb.numpy()
            else:
                arrays["digest_B"] = np.array(orf.input_digest(fa, fb))
            arrays[f"out_{case}"] = flat.numpy()
        save("corr", arrays)

        arrays = {}
        for k in orf.POOL_CASES:
            x = orf.pool_input(k)
            pooled, mi, mj, mk, ml = ref.modules.maxpool4d(x.unsqueeze(1), k)
            arrays[f"x_{k}"], arrays[f"pooled_{k}"] = x.numpy(), pooled[:, 0].numpy()
            arrays[f"delta_{k}"] = torch.stack([mi, mj, mk, ml])[:, :, 0].to(torch.int8).numpy()
        x = orf.mm_input()
        arrays["mm_x"], arrays["mm_y"] = x.numpy(), ref.ncn_model.MutualMatching(x.unsqueeze(1))[:, 0].numpy()
        for case, (shape, dim) in orf.L2_CASES.items():
            x = orf.l2_input(case)
            arrays[f"l2_x_{case}"], arrays[f"l2_y_{case}"] = x.numpy(), ref.modules.L2Normalize(x, dim).numpy()
        save("pool_mm_l2", arrays)

        arrays = {}
        for case, (ci, co, k, has_bias) in orf.CONV_CASES.items():
            w, bias = orf.conv_weights(case)
            layer = ref.conv4d.Conv4d(ci, co, k, bias=has_bias)
            layer.load_state_dict({"weight": w} if bias is None else {"weight": w, "bias": bias}, strict=True)
            arrays[f"w_{case}"] = w.numpy()
            if bias is not None:
                arrays[f"bias_{case}"] = bias.numpy()
            for vol in orf.CONV_VOLUMES:
                x = orf.conv_input(case, vol)
                y = layer(x)
                table[f"conv_{case}_{vol}"] = orf.rel_err(y, orf.conv4d64(x, w, bias))
                arrays[f"x_{case}_{vol}"], arrays[f"y_{case}_{vol}"] = x.numpy(), y.numpy()
        save("conv4d", arrays)

        arrays = {"x": orf.nc_input().numpy()}
        for case, c in orf.NC_CASES.items():
            sd = orf.nc_weights(case)
            net = ref.ncn_model.NeighConsensus(use_cuda=False, kernel_sizes=c["kernel_sizes"], channels=c["channels"],
                                               symmetric_mode=c["symmetric_mode"])
            net.load_state_dict(sd, strict=True)
            y = net(orf.nc_input().unsqueeze(1))[:, 0].contiguous()
            y64 = orf.neigh_consensus64(orf.nc_input(), case)
            table[f"nc_{case}"] = orf.rel_err(y, y64)
            print(f"nc_{case}: share of non-zero cells {float((y64 > 0).double().mean()):.3f}")
            arrays[f"y_{case}"] = y.numpy()
            for key, v in sd.items():
                arrays[f"{case}.{key}"] = v.numpy()
        save("nc", arrays)

        arrays = {}
        for ksize in (1, 2):
            x, delta = orf.match_inputs(ksize)
            arrays[f"x_{ksize}"] = x.numpy()
            if delta is not None:
                arrays[f"delta_{ksize}"] = torch.stack(delta).to(torch.int8).numpy()
        for name, ksize, kw in orf.match_cases() + orf.coord_cases():
            x, delta = orf.match_inputs(ksize)
            out = ref.extract.corr_to_matches(x, delta4d=delta, **kw)
            for i, t in enumerate(out):
                arrays[f"{name}.{i}"] = t.numpy()
        for name, ksize, kw in orf.topk_cases():
            x, delta = orf.match_inputs(ksize)
            out = ref.extract.corr_to_matches_topk(x, delta4d=delta, **kw)
            for i, t in enumerate(out):
                arrays[f"{name}.{i}"] = t.numpy()
        save("matches", arrays)

    # rounded UP to three digits: the recorded bound must not fall below the measured error
    up = lambda v: float(f"{v:.2e}") if float(f"{v:.2e}") >= v else float(f"{v:.2e}") + 10 ** (np.floor(np.log10(v)) - 2)
    print("REF_ERR = {" + ", ".join(f'"{k}": {up(v):.3g}' for k, v in table.items()) + "}")


if __name__ == "__main__":
    main()
