"""CPU test of the pooled path's launch plan: what mkb_pool_supported and mkb_pool_step_workspace_bytes answer over a grid of
table shapes and under every setting of the two per-call switches, against values recorded from the library before the
planner was restructured.  Neither call touches the device (the table pointers are only looked at for their alignment).

    python tests/test_host_pool_plan.py        # re-record tests/golden/pool_plan.npz from the library _hip.lib() loads
"""
import itertools
import os
import pathlib

import numpy as np

MODELS = ["TransE", "RotatE", "ComplEx", "DistMult", "pRotatE"]
# hidden dims across the units-per-lane / waves-per-workgroup boundaries, odd ones and ones not divisible by 4 included
DIMS = [3, 30, 64, 100, 255, 256, 257, 500, 512, 513, 1000, 1024, 1025, 1026, 2048, 2049, 2052, 4096, 4097]
BATCHES = [1, 7, 60, 256, 1000, 1024, 4096]                 # below 64, not a multiple of 8, 1000
SIZES = [1, 16, 64, 192, 256, 512, 513, 1024, 1025]         # K: 192 = 3 halves, 512 / 513 = the two-pass boundary
RELATIONS = [11, 237]                                       # few (relation-gradient copies) and many
ENT_POINTERS = [0x40000000, 0x40000004]                     # a 16-byte aligned and a misaligned table
NO_MFMA = [None, "1", "0"]
DENSE = [None, "0", "1"]
SHAPE = tuple(len(a) for a in (MODELS, DIMS, BATCHES, SIZES, RELATIONS, ENT_POINTERS, NO_MFMA, DENSE))


def _set(name, value):
    if value is None:
        os.environ.pop(name, None)
    else:
        os.environ[name] = value


def answers():
    """(supported [int8], workspace bytes [int64]) of the loaded library over the grid, in SHAPE order"""
    from mkb_amd import _hip

    lib = _hip.lib()
    saved = {k: os.environ.get(k) for k in ("MKB_POOL_NO_MFMA", "MKB_POOL_DENSE")}
    supported, nbytes = np.zeros(SHAPE, np.int8), np.zeros(SHAPE, np.int64)
    try:
        for idx in itertools.product(*(range(n) for n in SHAPE)):
            model, d, B, K, n_rel, ent = (a[i] for a, i in zip((MODELS, DIMS, BATCHES, SIZES, RELATIONS, ENT_POINTERS), idx))
            _set("MKB_POOL_NO_MFMA", NO_MFMA[idx[6]])
            _set("MKB_POOL_DENSE", DENSE[idx[7]])
            de = 2 * d if model in ("RotatE", "ComplEx") else d
            dr = 2 * d if model == "ComplEx" else d
            tb = _hip.Tables(_hip.MODEL_IDS[model], d, 14541, n_rel, de, dr, ent, 0x50000000, 0x50100000, 12.0, 0.5)
            supported[idx] = lib.mkb_pool_supported(tb, B, K)
            nbytes[idx] = lib.mkb_pool_step_workspace_bytes(tb, B, K)
    finally:
        for k, v in saved.items():
            _set(k, v)
    return supported, nbytes


def test_pool_plan_answers_match_the_recorded_ones(golden):
    g = golden("pool_plan.npz")
    assert tuple(g["shape"]) == SHAPE, "the grid of this module and the recorded one differ: re-record from the same commit"
    supported, nbytes = answers()
    # the grid reaches both answers, and every supported shape has a workspace
    assert 0 < int(g["supported"].sum()) < g["supported"].size
    assert (g["nbytes"][g["supported"] != 0] > 0).all()
    bad = np.argwhere((supported != g["supported"]) | (nbytes != g["nbytes"]))
    assert len(bad) == 0, (f"{len(bad)} of {supported.size} answers differ; first (model, dim, B, K, relations, ent, NO_MFMA, DENSE) "
                           f"index {bad[0].tolist()}: supported {supported[tuple(bad[0])]} vs {g['supported'][tuple(bad[0])]}, "
                           f"bytes {nbytes[tuple(bad[0])]} vs {g['nbytes'][tuple(bad[0])]}")


if __name__ == "__main__":
    import sys

    root = pathlib.Path(__file__).resolve().parent.parent
    sys.path.insert(0, str(root))
    s, n = answers()
    out = root / "tests" / "golden" / "pool_plan.npz"
    np.savez_compressed(out, shape=np.array(SHAPE, np.int64), supported=s, nbytes=n)
    print(f"{out}: {s.size} answers, {int(s.sum())} supported, {out.stat().st_size} bytes")
