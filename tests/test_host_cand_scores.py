"""CPU (-m "not gpu") tests of the host part of candidate scoring in any slot: the C ABI (include/mkb_hip.h, "candidate lists in any
one slot", under ABI 8) exports mkb_cand_score_fwd / mkb_cand_score_bwd_workspace_bytes / mkb_cand_score_bwd with the declared
signatures and refuses bad arguments before any launch; and ``Distillation.distillation_candidates`` holds, part by part, the
rows and lists that ``distillation_tensors`` writes out."""
import ctypes
import re

import pytest
import torch

DECLARED = {
    "mkb_cand_score_fwd": ("int", ["const mkb_tables_t *tb", "const int64_t *sample", "const int64_t *cand", "int64_t B", "int64_t M",
                                   "int part", "float *score", "void *stream"]),
    "mkb_cand_score_bwd_workspace_bytes": ("int64_t", ["const mkb_tables_t *tb", "int64_t B", "int64_t M", "int part"]),
    "mkb_cand_score_bwd": ("int", ["const mkb_tables_t *tb", "const mkb_grads_t *gr", "const int64_t *sample", "const int64_t *cand",
                                   "int64_t B", "int64_t M", "int part", "const float *dscore", "void *ws", "int64_t ws_bytes",
                                   "void *stream"]),
}


def test_candidate_symbols_signatures_and_abi():
    from conftest import ROOT
    from mkb_amd import _hip

    header = (ROOT / "include" / "mkb_hip.h").read_text()
    assert re.search(r"#define MKB_ABI_VERSION 9\b", header) and _hip.ABI_VERSION == 9
    assert re.search(r"typedef enum \{ MKB_PART_HEAD = 0, MKB_PART_RELATION = 1, MKB_PART_TAIL = 2 \} mkb_part_t;", header)
    assert (_hip.PART_HEAD, _hip.PART_RELATION, _hip.PART_TAIL) == (0, 1, 2)
    lib = ctypes.CDLL(str(ROOT / "mkb_amd" / "libmkb_hip.so"))
    c = ctypes

    def ctype(param):
        if param == "const mkb_tables_t *tb":
            return c.POINTER(_hip.Tables)
        if param == "const mkb_grads_t *gr":
            return c.POINTER(_hip.Grads)
        return c.c_void_p if "*" in param else {"int64_t": c.c_int64, "int": c.c_int}[param.split()[0]]

    for name, (res, params) in DECLARED.items():
        decl = re.search(r"\b%s %s\(([^)]*)\);" % (res, name), header)
        assert decl, name
        assert [" ".join(a.split()) for a in decl.group(1).split(",")] == params, name
        assert _hip._SIGNATURES[name] == ({"int": c.c_int, "int64_t": c.c_int64}[res], [ctype(p) for p in params]), name
        assert hasattr(lib, name) and name in _hip.EXPORTED_SYMBOLS, name
    assert _hip.lib().mkb_abi_version() == 9


@pytest.mark.parametrize("part", [0, 1, 2])
def test_candidate_abi_rejects_bad_arguments_before_any_launch(part):
    """Pointers that are never dereferenced: every call fails validation first (or has B == 0 and launches nothing)."""
    from mkb_amd import _hip

    lib = _hip.lib()
    p = ctypes.c_void_p(0x10000)
    tb = _hip.Tables(_hip.MODEL_IDS["RotatE"], 8, 100, 3, 16, 8, p, p, p, 6.0, 1.0)
    bad_model = _hip.Tables(99, 8, 100, 3, 16, 8, p, p, p, 6.0, 1.0)
    # (2 + 4) * entity_dim * 4 bytes against 64 KB: 2730 floats fit, 2731 do not
    fits = _hip.Tables(_hip.MODEL_IDS["TransE"], 2730, 100, 3, 2730, 2730, p, p, p, 6.0, 1.0)
    long_rows = _hip.Tables(_hip.MODEL_IDS["TransE"], 2731, 100, 3, 2731, 2731, p, p, p, 6.0, 1.0)
    protate = _hip.Tables(_hip.MODEL_IDS["pRotatE"], 8, 100, 3, 8, 8, p, p, p, 6.0, 1.0)
    grads, no_modulus = _hip.Grads(p, p, p), _hip.Grads(p, p, None)
    B, M = 4, 5
    need = lib.mkb_cand_score_bwd_workspace_bytes(tb, B, M, part)
    assert need >= 4 * B * M * 4 and need % 256 == 0  # at least the pair list twice, keys and values
    for b in (0, -1, 1 << 31):
        assert lib.mkb_cand_score_bwd_workspace_bytes(tb, b, M, part) == 0
    for args in [(None, B, M, part), (tb, B, 0, part), (tb, B, -2, part), (tb, B, M, 3), (tb, B, M, -1), (tb, 1 << 20, 1 << 20, part)]:
        assert lib.mkb_cand_score_bwd_workspace_bytes(*args) == 0, args[1:]
    ws = ctypes.c_void_p(0x100000)  # 256-byte aligned

    def refused(rc, what):
        assert rc == _hip.ERR_INVALID, what
        assert lib.mkb_last_error(), what

    def fwd(tb=tb, sample=p, cand=p, B=B, M=M, part=part, score=p):
        return lib.mkb_cand_score_fwd(tb, sample, cand, B, M, part, score, None)

    def bwd(tb=tb, gr=grads, sample=p, cand=p, B=B, M=M, part=part, dscore=p, ws=ws, ws_bytes=need):
        return lib.mkb_cand_score_bwd(tb, gr, sample, cand, B, M, part, dscore, ws, ws_bytes, None)

    common = [dict(tb=None), dict(tb=bad_model), dict(sample=None), dict(cand=None), dict(B=-1), dict(B=1 << 31), dict(M=0), dict(M=-3),
              dict(B=1 << 20, M=1 << 20), dict(part=3), dict(part=-1)]
    for kw in common + [dict(score=None)]:
        refused(fwd(**kw), ("fwd", kw))
    for kw in common + [dict(gr=None), dict(gr=_hip.Grads(None, p, p)), dict(gr=_hip.Grads(p, None, p)), dict(dscore=None), dict(ws=None),
                        dict(ws_bytes=need - 1), dict(ws_bytes=0), dict(ws=ctypes.c_void_p(0x100010)), dict(tb=protate, gr=no_modulus)]:
        refused(bwd(**kw), ("bwd", kw))
    # a valid call that launches nothing
    assert fwd(B=0) == 0 and bwd(B=0) == 0 and bwd(B=0, ws=None, ws_bytes=0) == 0
    # rows too long for the LDS staging: the caller keeps the block route.  (One float less: accepted -- B == 0 launches nothing.)
    assert fwd(tb=long_rows) == _hip.ERR_UNSUPPORTED and bwd(tb=long_rows) == _hip.ERR_UNSUPPORTED
    assert fwd(tb=fits, B=0) == 0 and bwd(tb=fits, B=0) == 0


class _ListSampling:
    """A sampler with fixed per-row lists (teacher ids and their student ids), supervised or not."""
    depends_on_teacher = False

    def __init__(self, lists, supervised):
        self.lists, self.supervised, self.calls = lists, supervised, 0

    def get(self, **kwargs):
        self.calls += 1
        return self.lists


@pytest.mark.parametrize("supervised", [False, True])
def test_distillation_candidates_rebuild_the_distillation_tensors(supervised):
    """On the CPU: substituting each part's lists into its rows gives exactly the [n, m, 3] tensors of ``distillation_tensors``,
    which in turn are what the part's definition says (rows kept by the availability rule, the ground truth in the last slot of a
    supervised sampler); one ``sampling.get`` per call of either."""
    from mkb_amd import distillation

    g = torch.Generator().manual_seed(3)
    t_ents, t_rels = {f"e{i}": i for i in range(12)}, {f"r{i}": i for i in range(5)}
    s_ents = {f"e{i}": (7 * i + 2) % 9 for i in range(9)}  # e9 .. e11 unknown to the student, ids permuted
    s_rels = {f"r{i}": 3 - i for i in range(4)}            # r4 unknown
    B, me, mr = 10, 4, 3
    sample = torch.stack([torch.randint(12, (B,), generator=g), torch.randint(5, (B,), generator=g), torch.randint(12, (B,), generator=g)], 1)
    sample[0] = torch.tensor([1, 2, 3])    # every part shared
    sample[1] = torch.tensor([10, 2, 3])   # head unshared
    sample[2] = torch.tensor([1, 4, 3])    # relation unshared
    sample[3] = torch.tensor([1, 2, 11])   # tail unshared
    ent_s = torch.tensor([s_ents.get(f"e{i}", -1) for i in range(12)])
    rel_s = torch.tensor([s_rels.get(f"r{i}", -1) for i in range(5)])
    head_t, tail_t = torch.randint(9, (B, me), generator=g), torch.randint(9, (B, me), generator=g)
    rel_t = torch.randint(4, (B, mr), generator=g)
    lists = (head_t, rel_t, tail_t, ent_s[head_t], rel_s[rel_t], ent_s[tail_t])
    sampling = _ListSampling(lists, supervised)
    proc = distillation.Distillation(t_ents, s_ents, t_rels, s_rels, sampling=sampling)
    cands = proc.distillation_candidates(sample)
    assert sampling.calls == 1
    tensors = proc.distillation_tensors(sample)
    assert sampling.calls == 2
    assert tuple(cands) == tuple(tensors) == ("head", "relation", "tail")
    ok = (ent_s[sample[:, 0]] >= 0, rel_s[sample[:, 1]] >= 0, ent_s[sample[:, 2]] >= 0)
    mapped = torch.stack([ent_s[sample[:, 0]], rel_s[sample[:, 1]], ent_s[sample[:, 2]]], 1)
    for col, part in enumerate(("head", "relation", "tail")):
        rows_t, cand_t, rows_s, cand_s = cands[part]
        keep = ok[0] & ok[1] & ok[2] if supervised else ok[(col + 1) % 3] & ok[(col + 2) % 3]
        assert 0 < int(keep.sum()) < B
        want_t, want_s = lists[col][keep].clone(), lists[3 + col][keep].clone()
        if supervised:
            want_t[:, -1], want_s[:, -1] = sample[keep, col], mapped[keep, col]
        assert rows_t.dtype == cand_t.dtype == rows_s.dtype == cand_s.dtype == torch.int64
        assert torch.equal(rows_t, sample[keep]) and torch.equal(rows_s, mapped[keep])
        assert torch.equal(cand_t, want_t) and torch.equal(cand_s, want_s)
        for rows, cand, block in ((rows_t, cand_t, tensors[part][0]), (rows_s, cand_s, tensors[part][1])):
            built = rows.unsqueeze(1).repeat(1, cand.shape[1], 1)
            built[:, :, col] = cand
            assert block.shape == (int(keep.sum()), cand.shape[1], 3) and block.is_contiguous() and torch.equal(built, block)


def test_score_candidates_validates_and_refuses_the_cpu():
    from mkb_amd import models

    m = models.RotatE(hidden_dim=4, entities={i: i for i in range(5)}, relations={0: 0}, gamma=1)
    s, c = torch.tensor([[0, 0, 1]]), torch.tensor([[1, 2]])
    with pytest.raises(ValueError, match="part must"):
        m.score_candidates(s, c, "tail-batch")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.score_candidates(s, c, "head")
