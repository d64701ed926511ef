"""Case table, seeded problems and float64 expectations for the route tests of the filtered ranking and top k
(tests/test_host_rank_routes.py, tests/test_gpu_rank_routes.py).  Host code only: nothing here touches the device.

``run_rank`` (mkb_amd/csrc/rank.hip) sends the all-entity score block down one of three routes and the lane route picks one of
four instantiations by row width.  ``CASES`` holds the smallest shapes that still select each of them, both sides of every
selection edge, and the entity counts at which the kernels' own strides come into play (one ragged 64-position tile, fewer
entities than slices, N % 4 != 0 on the matrix route, N around the 16-candidate slab and around rank_kernel's 8 x 64 stride).
"""
from __future__ import annotations

import functools
import zlib

import numpy as np
import torch

from oracle import ranking, scoring

GAMMA = 6.0
MODES = ("head-batch", "tail-batch")
DISTANCE_MODELS = ("TransE", "RotatE", "pRotatE")

# (model, hidden, N, R, B, n_true, route, instantiation).  n_true: random true triples drawn on top of the test triples and of the
# one filtered candidate per query and side.  Tables stay small: N <= 130 where a row exceeds 1024 floats, N <= 1030 otherwise.
CASES = [
    # ---- lane route, one unit per lane (units <= 512)
    ("pRotatE", 3, 1, 2, 1, 0, "lane", "kpt1"),
    ("RotatE", 31, 2, 3, 5, 4, "lane", "kpt1"),               # hidden 31: below the tile route's 32
    ("TransE", 63, 17, 4, 8, 40, "lane", "kpt1"),             # entity_dim 63: below the tile route's 64
    ("DistMult", 512, 33, 5, 5, 60, "lane", "kpt1"),
    ("pRotatE", 8, 512, 7, 9, 600, "lane", "kpt1"),           # N = 512: one full 8 x 64 stride of rank_kernel
    ("TransE", 24, 513, 6, 8, 600, "lane", "kpt1"),           # N = 513: one entity past it
    ("pRotatE", 8, 1030, 3, 72, 900, "lane", "kpt1"),         # 9 query tiles -> 57 slices of 19 entities: a full slab of 16 + 3
    ("pRotatE", 3, 17, 2, 4096, 30, "lane", "kpt1"),          # 512 query tiles -> ONE slice of 17 entities: a full slab + 1
    ("DistMult", 5, 16, 2, 4090, 30, "lane", "kpt1"),         # ... exactly one slab, ragged last query tile
    ("TransE", 7, 15, 3, 4089, 30, "lane", "kpt1"),           # ... one short slab
    ("ComplEx", 8, 129, 5, 28, 200, "lane", "kpt1"),          # B = 28: below the matrix route's 32
    ("DistMult", 12, 128, 4, 32, 200, "lane", "kpt1"),        # entity_dim 12: below the matrix route's 16
    ("DistMult", 16, 127, 4, 34, 200, "lane", "kpt1"),        # B % 4 != 0 keeps the lane route
    # ---- lane route, two units per lane, 8 waves (units <= 1024)
    ("pRotatE", 513, 130, 3, 9, 150, "lane", "kpt2w8"),
    ("RotatE", 1022, 33, 2, 1, 50, "lane", "kpt2w8"),
    ("ComplEx", 300, 17, 7, 7, 40, "lane", "kpt2w8"),
    ("DistMult", 1000, 17, 3, 5, 40, "lane", "kpt2w8"),
    ("TransE", 1023, 130, 5, 5, 150, "lane", "kpt2w8"),
    # ---- lane route, two units per lane, 16 waves (units <= 2048)
    ("pRotatE", 1025, 2, 2, 8, 3, "lane", "kpt2w16"),
    ("RotatE", 2046, 17, 3, 9, 40, "lane", "kpt2w16"),
    ("ComplEx", 1024, 130, 4, 31, 200, "lane", "kpt2w16"),
    ("DistMult", 2048, 33, 6, 30, 80, "lane", "kpt2w16"),
    ("TransE", 2047, 130, 2, 1, 100, "lane", "kpt2w16"),
    # ---- lane route, four units per lane (units <= 4096)
    ("pRotatE", 2049, 17, 5, 5, 40, "lane", "kpt4"),
    ("pRotatE", 4096, 130, 3, 9, 200, "lane", "kpt4"),
    ("RotatE", 2050, 33, 4, 8, 60, "lane", "kpt4"),
    ("RotatE", 4094, 130, 2, 5, 150, "lane", "kpt4"),
    ("ComplEx", 1025, 2, 3, 9, 4, "lane", "kpt4"),
    ("ComplEx", 2048, 130, 7, 8, 200, "lane", "kpt4"),
    ("DistMult", 4096, 1, 2, 9, 0, "lane", "kpt4"),
    ("DistMult", 4096, 130, 2, 9, 150, "lane", "kpt4"),
    ("TransE", 4095, 130, 6, 8, 200, "lane", "kpt4"),
    # ---- register-tile route (RotatE hidden % 4 == 0 and >= 32, TransE entity_dim % 4 == 0 and >= 64)
    ("RotatE", 32, 1, 2, 63, 0, "tile", "tile"),
    ("RotatE", 32, 65, 3, 65, 100, "tile", "tile"),
    ("RotatE", 32, 1030, 5, 65, 900, "tile", "tile"),         # 17 position tiles, the last one of 6 entities
    ("RotatE", 36, 63, 4, 64, 100, "tile", "tile"),
    ("RotatE", 2052, 64, 2, 65, 100, "tile", "tile"),
    ("RotatE", 4096, 130, 7, 1, 150, "tile", "tile"),
    ("TransE", 64, 65, 3, 1, 80, "tile", "tile"),
    ("TransE", 64, 513, 4, 63, 600, "tile", "tile"),
    ("TransE", 68, 130, 5, 65, 200, "tile", "tile"),
    ("TransE", 4096, 63, 2, 63, 100, "tile", "tile"),
    ("TransE", 4096, 64, 6, 64, 100, "tile", "tile"),
    # ---- matrix-core route (ComplEx / DistMult, B % 4 == 0 and >= 32, entity_dim % 4 == 0 and >= 16)
    ("ComplEx", 8, 1, 2, 32, 0, "matrix", "f32tile64"),
    ("ComplEx", 8, 2, 3, 36, 4, "matrix", "f32tile64"),
    ("DistMult", 16, 3, 2, 32, 6, "matrix", "f32tile64"),
    ("DistMult", 16, 5, 4, 36, 10, "matrix", "f32tile64"),
    ("ComplEx", 8, 127, 5, 36, 200, "matrix", "f32tile64"),
    ("DistMult", 16, 128, 6, 32, 200, "matrix", "f32tile64"),
    ("ComplEx", 8, 129, 7, 32, 200, "matrix", "f32tile64"),
    ("DistMult", 4096, 129, 3, 32, 200, "matrix", "f32tile64"),
    # the planner gives the 128-row bf16x3 tiles only from 24 of them on (gemm_plan.h): three row tiles x nine column tiles
    ("ComplEx", 8, 1029, 4, 384, 900, "matrix", "bf16x3"),
    ("DistMult", 16, 1030, 5, 384, 900, "matrix", "bf16x3"),
    ("ComplEx", 256, 1027, 3, 384, 900, "matrix", "bf16x3"),
]

FAMILIES = ("lane", "tile", "matrix")


def case_id(case) -> str:
    model, hidden, N, R, B = case[:5]
    return f"{model}-h{hidden}-N{N}-R{R}-B{B}-{case[7]}"


def units_of(model: str, hidden: int) -> int:
    """The row width the lane route and the width limit count in: hidden for RotatE, entity_dim otherwise."""
    return hidden if model == "RotatE" else scoring.dims(model, hidden)[0]


def route_of(case):
    """-> (route, instantiation): the conditions of ``run_rank`` restated (mkb_amd/csrc/rank.hip; the workspace of
    ``_hip.Workspace`` is 256-byte aligned and the tables come from torch's allocator, so the alignment terms always hold).
    Used only to check that ``CASES`` covers the table."""
    model, hidden, N, _, B = case[:5]
    entity_dim = scoring.dims(model, hidden)[0]
    # rank.hip:475-478 -- the register tile for the complex-modulus pair function and TransE
    if model == "RotatE" and hidden % 4 == 0 and hidden >= 32 and N < (1 << 30):
        return "tile", "tile"
    if model == "TransE" and entity_dim % 4 == 0 and entity_dim >= 64 and N < (1 << 30):
        return "tile", "tile"
    # rank.hip:496-499 -- one product on the matrix cores
    if model in ("ComplEx", "DistMult"):
        npad = (N + 3) & ~3
        if B % 4 == 0 and entity_dim % 4 == 0 and entity_dim >= 16 and B >= 32 and npad < (1 << 30):
            # gemm_plan.h:79-94 -- M = B, N = npad, K = lda = ldb = entity_dim, max_ks = 1, default switches
            tiles128 = ((B + 127) // 128) * ((npad + 127) // 128)
            fits32 = B * entity_dim * 4 < (1 << 31) and N * entity_dim * 4 < (1 << 31)
            return "matrix", ("bf16x3" if tiles128 >= 24 and fits32 else "f32tile64")
    # rank.hip:520-524 -- lanes own dims: 1024 lanes x 1, 512 x 2, 1024 x 2, 1024 x 4 units
    units = units_of(model, hidden)
    assert units <= 4096
    return "lane", ("kpt1" if units <= 512 else "kpt2w8" if units <= 1024 else "kpt2w16" if units <= 2048 else "kpt4")


def lane_slices(case):
    """(slices, entities per slice) of the lane route's grid (rank.hip:515-518)."""
    N, B = case[2], case[4]
    tiles = (B + 7) // 8
    slices = min(max((512 + tiles - 1) // tiles, 1), N)
    return slices, (N + slices - 1) // slices


# ------------------------------------------------------------------------------------------------------------------ problems
def _tables(model, hidden, N, R, rs):
    de, dr = scoring.dims(model, hidden)
    rng = (GAMMA + 2.0) / hidden if model in DISTANCE_MODELS else 1.0
    ent = rs.uniform(-rng, rng, size=(N, de)).astype(np.float32)
    rel = rs.uniform(-rng, rng, size=(R, dr)).astype(np.float32)
    modulus = np.array([[0.5 * (GAMMA + 2.0) / hidden]], dtype=np.float32) if model in ("RotatE", "pRotatE") else None
    return ent, rel, modulus


class Problem:
    """Seeded tables, test triples and true triples of one case.

    Where N >= 8 five ids c1 < c2 < t < c3 < c4 share ONE entity row (exact copies of t's), as do two further ids p < q.  The first
    queries have t as their target: (t, r, t) on both sides, then -- B permitting -- (t, r, x) on the head side and (y, r, t) on the
    tail side.  For those queries c2 and c3 are made filtered candidates and c1, c4 stay candidates: c1 must count before the
    target, c2 must be taken back (it was counted), c3 must NOT be taken back (it never was), c4 must not count.  No other test
    or true triple touches the seven planted ids."""

    def __init__(self, case):
        model, hidden, N, R, B, n_true = case[:6]
        self.case, self.model, self.hidden, self.N, self.R, self.B = case, model, hidden, N, R, B
        rs = np.random.RandomState(zlib.crc32(case_id(case).encode()) & 0x7FFFFFFF)
        self.ent, self.rel, self.modulus = _tables(model, hidden, N, R, rs)
        self.planted = None
        pool = np.arange(N)
        if N >= 8:
            ids = np.sort(rs.choice(N, size=7, replace=False))
            rs_pick = rs.permutation(7)
            group = np.sort(ids[rs_pick[:5]])
            p, q = np.sort(ids[rs_pick[5:]])
            c1, c2, t, c3, c4 = (int(v) for v in group)
            self.planted = dict(c1=c1, c2=c2, t=t, c3=c3, c4=c4, p=int(p), q=int(q))
            for c in (c1, c2, c3, c4):
                self.ent[c] = self.ent[t]
            self.ent[q] = self.ent[p]
            pool = np.setdiff1d(pool, ids)
        triples = np.stack([rs.choice(pool, size=B), rs.randint(R, size=B), rs.choice(pool, size=B)], 1).astype(np.int64)
        true = [triples]
        self.tie_queries = {"head-batch": [], "tail-batch": []}
        if self.planted is not None:
            t, c2, c3 = self.planted["t"], self.planted["c2"], self.planted["c3"]
            triples[0, 0] = triples[0, 2] = t
            self.tie_queries["head-batch"].append(0)
            self.tie_queries["tail-batch"].append(0)
            if B >= 3:
                triples[1, 0] = t
                triples[2, 2] = t
                self.tie_queries["head-batch"].append(1)
                self.tie_queries["tail-batch"].append(2)
            for i in self.tie_queries["head-batch"]:
                true.append(np.array([[c2, triples[i, 1], triples[i, 2]], [c3, triples[i, 1], triples[i, 2]]]))
            for i in self.tie_queries["tail-batch"]:
                true.append(np.array([[triples[i, 0], triples[i, 1], c2], [triples[i, 0], triples[i, 1], c3]]))
        # every query filters at least one candidate on each side (N = 1 has none to filter)
        if len(pool) >= 2:
            other_h = np.array([rs.choice(pool[pool != h]) for h in triples[:, 0]])
            other_t = np.array([rs.choice(pool[pool != t]) for t in triples[:, 2]])
            true.append(np.stack([other_h, triples[:, 1], triples[:, 2]], 1))
            true.append(np.stack([triples[:, 0], triples[:, 1], other_t], 1))
        if n_true:
            true.append(np.stack([rs.choice(pool, size=n_true), rs.randint(R, size=n_true), rs.choice(pool, size=n_true)], 1))
        self.triples = triples
        self.true = np.unique(np.concatenate(true).astype(np.int64), axis=0)
        self.keys = ranking.true_key_set(self.true, N, R)

    def tables(self, dtype):
        """``scoring.Tables`` in ``dtype`` (its arithmetic is dtype-agnostic)."""
        mod = None if self.modulus is None else torch.from_numpy(self.modulus).to(dtype)
        return scoring.Tables(self.model, self.hidden, GAMMA, torch.from_numpy(self.ent).to(dtype), torch.from_numpy(self.rel).to(dtype), mod)

    def target(self, mode):
        return self.triples[:, 0 if mode == "head-batch" else 2]

    def filtered(self, mode):
        """bool [B, N]: the candidates the filter removes (the other true triples; never the target)."""
        _, bias = ranking.candidates(self.triples, self.keys, self.N, self.R, mode)
        return bias != 0


@functools.lru_cache(maxsize=None)
def problem(case) -> Problem:
    return Problem(case)


def score_block(tb, triples, N, mode, chunk=4):
    """[n, N] scores of every entity in order by ``oracle.scoring.score`` in the dtype of ``tb`` (RotatE with sqrt(re^2 + im^2):
    the kernels' form, ~1 ulp per term from the reference's stack -> norm)."""
    s_all = torch.as_tensor(np.asarray(triples, dtype=np.int64).reshape(-1, 3))
    everyone = torch.arange(N, dtype=torch.int64)
    out = []
    with torch.no_grad():
        for lo in range(0, len(s_all), chunk):
            s = s_all[lo: lo + chunk]
            out.append(scoring.score(tb, s, everyone.unsqueeze(0).expand(len(s), -1), mode, fast_norm=True))
    return torch.cat(out).numpy()


def ranks_from_scores(scores, filtered, target):
    """The filtered rank under the order of rank_order.h -- NaN first, then higher score, then lower id -- counted on ``scores``
    [n, N] with the ``filtered`` columns left out: 1 + the candidates that come before the target."""
    n, N = scores.shape
    ids = np.arange(N)[None, :]
    st = scores[np.arange(n), target][:, None]
    tg = np.asarray(target)[:, None]
    a_nan, b_nan = np.isnan(scores), np.isnan(st)
    with np.errstate(invalid="ignore"):
        plain = (scores > st) | ((scores == st) & (ids < tg))
    before = np.where(a_nan | b_nan, a_nan & (~b_nan | (ids < tg)), plain)
    before &= ~filtered & (ids != tg)
    return 1 + before.sum(axis=1)


@functools.lru_cache(maxsize=None)
def expected(case):
    """-> {mode: (float64 scores [B, N], filtered ranks [B] counted on them, filtered [B, N] bool)}."""
    pb = problem(case)
    tb = pb.tables(torch.float64)
    chunk = 4 if scoring.dims(pb.model, pb.hidden)[0] > 1024 else 64
    out = {}
    for mode in MODES:
        s = score_block(tb, pb.triples, pb.N, mode, chunk=chunk)
        f = pb.filtered(mode)
        out[mode] = (s, ranks_from_scores(s, f, pb.target(mode)), f)
    return out


# ---------------------------------------------------------------------------------------------------------------- tolerance
ERR_FACTOR = 8.0


@functools.lru_cache(maxsize=None)
def calibration(model, hidden):
    """-> (err_ref, typical term) on a block of 16 queries x 128 entities of the cases' distribution: err_ref = max |fp32
    oracle.scoring.score - float64 score| over both sides; the typical single term of a score is mean (gamma - score) / units for
    the distance models and rms(score) / sqrt(units) for ComplEx / DistMult."""
    rs = np.random.RandomState(zlib.crc32(f"calibration-{model}-{hidden}".encode()) & 0x7FFFFFFF)
    N, R, n = 128, 4, 16
    ent, rel, modulus = _tables(model, hidden, N, R, rs)
    triples = np.stack([rs.randint(N, size=n), rs.randint(R, size=n), rs.randint(N, size=n)], 1)
    err, blocks = 0.0, []
    for mode in MODES:
        both = []
        for dtype in (torch.float32, torch.float64):
            mod = None if modulus is None else torch.from_numpy(modulus).to(dtype)
            tb = scoring.Tables(model, hidden, GAMMA, torch.from_numpy(ent).to(dtype), torch.from_numpy(rel).to(dtype), mod)
            both.append(score_block(tb, triples, N, mode))
        err = max(err, float(np.abs(both[0].astype(np.float64) - both[1]).max()))
        blocks.append(both[1])
    s = np.concatenate(blocks)
    units = units_of(model, hidden)
    if model in DISTANCE_MODELS:
        term = float((GAMMA - s).mean()) / units
    else:
        term = float(np.sqrt((s * s).mean())) / np.sqrt(units)
    return err, term


# Largest device error / err_ref measured per route on the MI355X over CASES, where it exceeds the factor 8 with no defect behind
# it: the register tile sums a whole row's terms into two running fp32 sums per (query, entity) pair (4096 sequential adds at the
# widest row: RotatE hidden 4096, N = 130), the 64-row matrix-core kernel accumulates K two products at a time (DistMult hidden
# 4096, N = 129: 2048 sequential adds onto sums of ~30), and the bf16x3 kernel 192 times per 512 of K (ComplEx hidden 256,
# N = 1027: 8.7); torch's sums, which err_ref measures, are blocked and far shorter.  The lane route's tree reduction stays
# below 1.6 x err_ref.  These routes get 2 x their measured ratio, capped where the quarter-term condition would break.
MEASURED_RATIO = {"tile": 11.59, "matrix": 16.18}


def tolerance(model, hidden, route="lane") -> float:
    """What the device's scores may differ from float64 by: 8 x the reference arithmetic's own fp32 error (the device sums the same
    fp32 terms in another order; the matrix route drops only products below 2^-24 |a||b|, gemm_mfma.h).  The factor covers the
    order effects and the maximum over a larger block than the calibration's.  Routes whose honest error was measured above that
    (MEASURED_RATIO) take twice their measured ratio instead, and never more than a quarter of the typical single term."""
    err_ref, term = calibration(model, hidden)
    return min(max(ERR_FACTOR, 2.0 * MEASURED_RATIO.get(route, 0.0)) * err_ref, max(ERR_FACTOR * err_ref, 0.25 * term))


def band(case, mode):
    """(lo, hi) of ``oracle.ranking.rank_bounds`` on the float64 scores with eps = 2 x tolerance."""
    pb = problem(case)
    s, _, f = expected(case)[mode]
    target = pb.target(mode)
    biased = np.where(f, s[np.arange(pb.B), target][:, None] + ranking.FILTER_BIAS, s)
    return ranking.rank_bounds(s, biased, target, 2.0 * tolerance(pb.model, pb.hidden, case[6]))


def clear_share():
    """{route family: share of the (query, side) pairs of its cases whose band is one rank wide}."""
    n, clear = dict.fromkeys(FAMILIES, 0), dict.fromkeys(FAMILIES, 0)
    for case in CASES:
        for mode in MODES:
            lo, hi = band(case, mode)
            n[case[6]] += len(lo)
            clear[case[6]] += int((lo == hi).sum())
    return {fam: clear[fam] / n[fam] for fam in FAMILIES}
