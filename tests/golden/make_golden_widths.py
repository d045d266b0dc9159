#!/usr/bin/env python
"""Generate tests/golden/g10_net_widths.npz: the REFERENCE's OthelloResNet (its src/model/net.py, loaded by path from the
reference tree oracle/build_ref.py points at) at filter counts between and beyond the four its configurations use.

Run:  python tests/golden/make_golden_widths.py     (needs the reference tree; writes tests/golden/g10_net_widths.npz)

For seeds 0 and 42 and every net below: the reference's (log_p, v) on the 32 positions of g4_net.npz (8x8) or the inputs of
g7_net6.npz (6x6), the state-dict key names and one SHA-256 per tensor.  No weights are stored: the package's OthelloResNet
regenerates them from the seed and tests/test_net_widths_cpu.py checks the hashes.  Nothing of the reference's program text
enters the file.
"""
import hashlib
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.dirname(HERE))  # tests/
import build_ref  # noqa: E402
import oracle_lib as ol  # noqa: E402

NETS8 = ((2, 48), (3, 96), (2, 160), (2, 192), (4, 256))
NETS6 = ((2, 96), (2, 176), (2, 256))


def reference_net_class():
    path = os.path.join(build_ref.REF, "src", "model", "net.py")
    spec = importlib.util.spec_from_file_location("_reference_model_net", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.OthelloResNet


def main():
    RefNet = reference_net_class()
    pos = np.load(os.path.join(HERE, "g4_net.npz"))["pos"]
    x8 = torch.from_numpy(np.stack([ol.tensor(ol.board(s, o)) for s, o in pos]))
    x6 = torch.from_numpy(np.load(os.path.join(HERE, "g7_net6.npz"))["x"])
    out = {}
    for seed in (0, 42):
        for board, x, nets in ((8, x8, NETS8), (6, x6, NETS6)):
            for nb, nf in nets:
                torch.manual_seed(seed)
                net = RefNet(nb, nf, board_size=board).eval()
                with torch.no_grad():
                    logp, v = net(x)
                tag = "b%d_s%d_%dx%d" % (board, seed, nb, nf)
                out[tag + "_logp"] = logp.numpy()
                out[tag + "_v"] = v.numpy()
                sd = net.state_dict()
                out[tag + "_keys"] = np.array(list(sd.keys()))
                out[tag + "_sha"] = np.array([hashlib.sha256(t.detach().cpu().numpy().tobytes()).hexdigest()
                                              for t in sd.values()])
    path = os.path.join(HERE, "g10_net_widths.npz")
    np.savez_compressed(path, **out)
    print("g10: %d nets, %d bytes" % (len(out) // 4, os.path.getsize(path)))


if __name__ == "__main__":
    main()
