"""Writes tests/golden/randn_pin.npz: the bytes eegldm_randn gives for three (seed, offset, n) cases.  Run on the GPU with the library
the pin is to be taken from (EEGLDM_LIB=/path/to/libeegldm.so, set before eegldm is imported; default: the tree's own build):

    EEGLDM_LIB=... python tests/golden/make_randn_pin.py [--out FILE]

tests/test_gpu_resample.py compares a fresh draw with these bytes: the file was taken from a library built BEFORE Philox and the
Box-Muller quad moved into csrc/elementwise.h, so it pins that the move changed nothing."""
import argparse
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
# n <= 64; a quad-aligned length, one that ends inside a quad, a large offset (past 2^32 counters) and a key with high bits set
CASES = [(1234, 0, 64), (0x5EED + 7, 2 ** 33 + 5, 37), (0xC0FFEE0012345678, 123456789, 5)]


def draw(seed, offset, n):
    import torch
    import eegldm
    from eegldm._lib import check, lib, ptr
    ctx = eegldm.default_context(0)
    out = torch.empty(n, device="cuda:0", dtype=torch.float32)
    check(lib.eegldm_randn(ctx.h, ptr(out), n, seed, offset))
    return out.cpu().numpy()


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "randn_pin.npz"))
    args = ap.parse_args(argv)
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    arrays = {"cases": np.array(CASES, dtype=np.uint64)}
    for i, (seed, offset, n) in enumerate(CASES):
        arrays[f"out{i}"] = draw(seed, offset, n)
        assert np.isfinite(arrays[f"out{i}"]).all()
    np.savez(args.out, **arrays)
    from eegldm._lib import LIB_PATH
    print(f"wrote {args.out} from {LIB_PATH}")


if __name__ == "__main__":
    main()
