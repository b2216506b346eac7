"""Write tests/golden/adamw_bits.npz: what oard_adamw_step_ema (three steps) and oard_adamw_step_dev_ema (one accepted step) leave in
the parameters, the moments and the average, as uint32 bit patterns, per case of tests/test_adamw_bits.py.  Needs an MI355X and the
built library.

The file records the library it is run against, so it is regenerated ONLY to record a deliberate change of the AdamW arithmetic; the
committed one was written from the four hand-copied kernels (k_adamw, k_adamw_dev, k_adamw_ema, k_adamw_dev_ema) that preceded
`adamw_elem`.  Inputs are not stored: the test rebuilds them from the same CPU-generator seeds (make_inputs).

    python oracle/make_goldens_adamw.py [output.npz]"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import test_adamw_bits as T  # noqa: E402


def main(path):
    dev = torch.device("cuda:0")
    out = {}
    for amsgrad, gscale in T.CASES:
        key = T.case_key(amsgrad, gscale)
        host = T.run_host(amsgrad, gscale, True, dev)
        devt, out4 = T.run_dev(amsgrad, gscale, True, dev)
        for k in T.NAMES:
            out[f"host_{key}_{k}"] = T.bits(host[k])
            out[f"dev_{key}_{k}"] = T.bits(devt[k])
            assert np.isfinite(host[k].cpu().numpy()).all() and np.isfinite(devt[k].cpu().numpy()).all(), (key, k)
        out[f"dev_{key}_out4"] = T.bits(out4)
        print(f"{key}: out4 {out4.tolist()}")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    np.savez(path, **out)
    print(f"wrote {path}: {len(out)} arrays, {os.path.getsize(path)} bytes")
    assert os.path.getsize(path) < 64 * 1024


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else T.GOLDEN)
