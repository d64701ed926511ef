"""The case table of the Adam launches (mkb_amd/csrc/adam.hip, planned by mkb_amd/csrc/adam_plan.h), their hand-made streams and the
float64 reference they are held against.  tests/test_host_adam_routes.py checks the table on the host (every case takes the leaves
it claims, the reference is torch's float64 Adam, defect models move it); tests/test_gpu_adam_routes.py runs it on the device.

A case is one table [N, D] stepped T times.  Every step lists L row ids (a deterministic visiting schedule plus seeded random rows,
duplicates, one negative id and one id past the table), catches them up, reads them, writes their gradient rows and steps.  The same
stream runs through dense ``mkb_adam_step``, the plain row-lazy form (catch-up + ``mkb_adam_rows_step``), the advance form, the
advance form with a flush in mid-run and, where claimed, the ownership form: all must end with the same bits.  The dense result is
held against the element rule restated in float64 (``reference``), within ``ERR_FACTOR`` x the distance torch.optim.Adam on float32
CPU tensors keeps from it (``err_ref``), per table row and per quantity.

Claims are words of the plan as tests/test_host_adam_routes.py prints it, prefixed by the launch they are about: ``catch:`` the
per-step catch-up / advance launch over the L listed rows, ``flush:`` the closing whole-table launch, ``step:``
``mkb_adam_rows_step``.
"""
import collections
import functools
import zlib

import numpy as np
import torch

ERR_FACTOR = 4.0                      # the issue's k: the update term carries about twice torch's rounding; a factor two over that
EPS = 1e-8
LRS = (1e-3, 4e-4)                    # the rate of steps 1 .. T // 2, and of the steps after: a deferred step must use its own step's rate
G_SCALES = (1.0, 1e-3, 1e3, 1e-9)     # gradient scale of row r: G_SCALES[r % 4]; at 1e-9 eps dominates the denominator
P_SCALES = (1.0, 0.01)                # |p| of row r: p_scales[(r // 4) % 2]
GAPS = (0, 1, 2, 3, 4, 5, 7, 8, 9, 33)  # pending zero-gradient steps the schedule produces: the groups and remainders of the four-wide replay
RANDOM_ZONE = (200, 230)              # rows the seeded random part of every id list comes from
EXTRA_STEPS = (10, 11, 12)            # steps whose catch-up is followed by one more, of 1, rows-per-workgroup - 1 and + 1 ids
RIDER_STEP_OFFSET = 2                 # a rider has its own step count: the table's + 2
CATCH_THREADS, HOST_THREADS = 512, 256
QUANTITIES = ("p", "m", "v")

Case = collections.namedtuple("Case", "name D claims N L T off sweep betas rider own group p_scales")


def _case(name, D, claims, N=299, L=25, T=40, off=0, sweep=None, betas=(0.9, 0.999), rider=0, own=False, group=None, p_scales=P_SCALES):
    return Case(name, D, frozenset(claims), N, L, T, off, sweep, betas, rider, own, group or name.split("-")[0], p_scales)


# N = 299 = 12 L - 1: the built-in rule keeps the sweep off and takes the lean replay (kernel=lean); N = 300 = 12 L turns the sweep
# on and takes the four-wide replay (kernel=unroll); N = 300 with MKB_ADAM_SWEEP=0 is the four-wide replay without a window.  The
# width pairs alternate between the first and the last so that both replays walk every width with the schedule's exact gaps.
_U = dict(N=300, sweep="0")
CASES = [
    # float4: rows per workgroup 8 | 4 | 2 | 1, the headline row, 1 | 2 | 3 passes
    _case("f4-256", 256, {"catch:access=4", "catch:rpb=8", "catch:lanes=64", "catch:kernel=lean"}),
    _case("f4-260", 260, {"catch:access=4", "catch:rpb=4", "catch:lanes=128", "catch:kernel=lean"}),
    _case("f4-512", 512, {"catch:access=4", "catch:rpb=4", "catch:kernel=unroll", "catch:sweep=0"}, **_U),
    _case("f4-516", 516, {"catch:access=4", "catch:rpb=2", "catch:lanes=256", "catch:kernel=unroll"}, **_U),
    _case("f4-1024", 1024, {"catch:access=4", "catch:rpb=2", "flush:access=4", "flush:passes=1", "step:access=4", "step:passes=1"}),
    _case("f4-1028", 1028, {"catch:access=4", "catch:rpb=1", "catch:lanes=512", "flush:access=4", "flush:passes=2", "step:access=4",
                            "step:passes=2"}),
    _case("f4-2000", 2000, {"catch:access=4", "catch:rpb=1", "catch:passes=1", "catch:kernel=unroll", "catch:sweep=10"}, N=300),
    _case("f4-2048", 2048, {"catch:access=4", "catch:rpb=1", "catch:passes=1", "catch:kernel=unroll"}, **_U),
    _case("f4-2052", 2052, {"catch:access=4", "catch:rpb=1", "catch:passes=2", "catch:kernel=unroll", "own"}, own=True, **_U),
    _case("f4-4100", 4100, {"catch:access=4", "catch:passes=3", "flush:passes=5", "step:passes=5", "catch:kernel=lean"}),
    # float2: an even D that is no multiple of four
    _case("f2-126", 126, {"catch:access=2", "catch:epl=2", "catch:rpb=8", "catch:kernel=unroll"}, **_U),
    _case("f2-130", 130, {"catch:access=2", "catch:rpb=4", "catch:kernel=unroll"}, **_U),
    _case("f2-510", 510, {"catch:access=2", "catch:rpb=2", "flush:access=2", "flush:passes=1", "step:access=1"}),
    _case("f2-514", 514, {"catch:access=2", "catch:rpb=1", "flush:access=2", "flush:passes=2"}),
    _case("f2-1022", 1022, {"catch:access=2", "catch:rpb=1", "catch:passes=1", "catch:kernel=unroll"}, **_U),
    _case("f2-1026", 1026, {"catch:access=2", "catch:rpb=1", "catch:passes=2", "catch:kernel=unroll"}, **_U),
    _case("f2-2050", 2050, {"catch:access=2", "catch:passes=3", "catch:kernel=lean"}),
    # an odd D: two elements per lane taken one at a time, the row ends on a single element
    # Rows of one and three elements.  err_ref is a maximum over the row: here over one to three samples.  Over 40 steps torch's
    # float32 stays within one ulp of float64 on half of such rows (the cap of test_host_adam_routes.py), so they take 400 and 200
    # steps; and their |p| is ~1 and ~0.25, not ~0.01: a parameter of 0.01 moves by up to 0.28 over 400 steps, passes zero and ends
    # anywhere, its final ulp no longer the scale of the roundings it collected on the way -- the ratio of two such single samples
    # says nothing (a wide row's maximum over its elements does not have this problem: every other case keeps |p| ~ 0.01).
    _case("odd-1", 1, {"catch:access=1", "catch:epl=2", "catch:rpb=8", "step:access=1", "flush:access=1"}, T=400, p_scales=(1.0, 0.25)),
    _case("odd-3", 3, {"catch:access=1", "catch:rpb=8", "catch:kernel=unroll"}, T=200, p_scales=(1.0, 0.25), **_U),
    _case("odd-33", 33, {"catch:access=1", "catch:rpb=8", "catch:kernel=lean"}),
    _case("odd-255", 255, {"catch:access=1", "step:access=1", "step:passes=1"}, **_U),
    _case("odd-257", 257, {"catch:access=1", "step:access=1", "step:passes=2"}, **_U),
    _case("odd-1023", 1023, {"catch:access=1", "catch:rpb=1", "catch:passes=1"}),
    _case("odd-1025", 1025, {"catch:access=1", "catch:rpb=1", "catch:passes=2", "catch:kernel=unroll"}, **_U),
    # a multiple of four with every pointer one float off the 16-byte grid: the replay takes float2
    _case("offset-64", 64, {"catch:access=2", "catch:vec4=0", "catch:epl=2", "flush:access=2", "step:access=4"}, off=1),
    # unroll and sweep
    _case("sweep-rule-on", 36, {"catch:kernel=unroll", "catch:sweep=10"}, N=300),
    _case("sweep-rule-off", 36, {"catch:kernel=lean", "catch:sweep=0"}, N=299),
    _case("sweep-zero", 36, {"catch:kernel=unroll", "catch:sweep=0"}, N=300, sweep="0"),
    _case("sweep-forced", 36, {"catch:kernel=lean", "catch:sweep=43"}, N=299, sweep="7"),
    _case("sweep-forced-wide", 1028, {"catch:kernel=lean", "catch:sweep=43", "catch:rpb=1"}, N=299, sweep="7"),
    # riders: 4 | 5 | 37 * 64 + 3 floats, and one past the grid-stride cap of the 256-lane and of the 512-lane kernels
    _case("rider-4", 36, {"catch:rider_blocks=1", "step:rider_blocks=1", "flush:rider_blocks=1"}, rider=4),
    _case("rider-5", 37, {"catch:rider_blocks=1", "step:rider_blocks=1"}, rider=5, **_U),
    _case("rider-2371", 130, {"catch:rider_blocks=2", "step:rider_blocks=3", "flush:rider_blocks=3"}, rider=37 * 64 + 3, N=300),
    _case("rider-cap256", 36, {"catch:rider_blocks=513", "step:rider_blocks=1024", "flush:rider_blocks=1024"}, rider=1024 * 256 * 4 + 5),
    _case("rider-cap512", 64, {"catch:rider_blocks=1024", "step:rider_blocks=1024"}, rider=1024 * 512 * 4 + 5, **_U),
    # betas (0.4, 0.9): the lerp weight 0.6 is above 0.5, where ATen switches formula
    _case("betas-130", 130, {"catch:access=2"}, betas=(0.4, 0.9)),
    _case("betas-2000", 2000, {"catch:access=4", "catch:kernel=unroll"}, betas=(0.4, 0.9), **_U),
]
CASE_IDS = [c.name for c in CASES]

# every leaf the table must reach: a set of words one case claims together
LEAVES = [
    {"catch:access=4", "catch:rpb=8"}, {"catch:access=4", "catch:rpb=4"}, {"catch:access=4", "catch:rpb=2"}, {"catch:access=4", "catch:rpb=1"},
    {"catch:access=4", "catch:passes=1", "catch:rpb=1"}, {"catch:access=4", "catch:passes=2"}, {"catch:access=4", "catch:passes=3"},
    {"catch:access=2", "catch:rpb=8"}, {"catch:access=2", "catch:rpb=4"}, {"catch:access=2", "catch:rpb=2"}, {"catch:access=2", "catch:rpb=1"},
    {"catch:access=2", "catch:passes=1", "catch:rpb=1"}, {"catch:access=2", "catch:passes=2"}, {"catch:access=2", "catch:passes=3"},
    {"catch:access=1", "catch:rpb=8"}, {"catch:access=1", "catch:passes=1", "catch:rpb=1"}, {"catch:access=1", "catch:passes=2"},
    {"catch:access=2", "catch:vec4=0", "step:access=4"},
    {"flush:access=4", "flush:passes=1"}, {"flush:access=4", "flush:passes=2"}, {"flush:access=2", "flush:passes=1"},
    {"flush:access=2", "flush:passes=2"}, {"flush:access=1"},
    {"step:access=4", "step:passes=1"}, {"step:access=4", "step:passes=2"}, {"step:access=1", "step:passes=1"}, {"step:access=1", "step:passes=2"},
    {"catch:kernel=unroll", "catch:sweep=10"}, {"catch:kernel=lean", "catch:sweep=0"}, {"catch:kernel=unroll", "catch:sweep=0"},
    {"catch:kernel=lean", "catch:sweep=43"}, {"own"},
    {"catch:rider_blocks=1"}, {"catch:rider_blocks=2"}, {"catch:rider_blocks=1024"}, {"step:rider_blocks=1024"}, {"flush:rider_blocks=1024"},
]
for _width in (4, 2, 1):  # both replays walk every access width
    LEAVES += [{f"catch:access={_width}", "catch:kernel=unroll"}, {f"catch:access={_width}", "catch:kernel=lean"}]

# (case below, case above, the word below, the word above): the claimed word flips across the edge
EDGES = [
    ("f4-256", "f4-260", "catch:rpb=8", "catch:rpb=4"), ("f4-512", "f4-516", "catch:rpb=4", "catch:rpb=2"),
    ("f4-1024", "f4-1028", "catch:rpb=2", "catch:rpb=1"), ("f4-2048", "f4-2052", "catch:passes=1", "catch:passes=2"),
    ("f2-126", "f2-130", "catch:rpb=8", "catch:rpb=4"), ("f2-510", "f2-514", "catch:rpb=2", "catch:rpb=1"),
    ("f2-1022", "f2-1026", "catch:passes=1", "catch:passes=2"), ("odd-1023", "odd-1025", "catch:passes=1", "catch:passes=2"),
    ("f4-1024", "f4-1028", "step:passes=1", "step:passes=2"), ("f4-1024", "f4-1028", "flush:passes=1", "flush:passes=2"),
    ("odd-255", "odd-257", "step:passes=1", "step:passes=2"), ("f2-510", "f2-514", "flush:passes=1", "flush:passes=2"),
    ("sweep-rule-off", "sweep-rule-on", "catch:kernel=lean", "catch:kernel=unroll"),
    ("sweep-rule-off", "sweep-rule-on", "catch:sweep=0", "catch:sweep=10"),
    ("rider-cap256", "rider-cap512", "catch:rider_blocks=513", "catch:rider_blocks=1024"),
]

# mkb_adam_step alone, and the eight tensors of one mkb_adam_step_multi launch as (n, step count)
DENSE_NS = (1, 2, 3, 4, 5, 1023, 1024, 1025, 2048 * 256 * 4 + 5)
DENSE_STEPS = 6
MULTI = ((1, 3), (3, 1), (1025, 7), (4, 2), (5, 65536), (1023, 4), (1024, 9), (37 * 64 + 3, 5))

# Largest measured (device deviation from float64) / err_ref per case group, on an MI355X (profiles/r27_adam_routes_errors.txt).
# The bound of the device test is ERR_FACTOR, derived in its docstring; this table records what was measured, it widens nothing.
MEASURED_RATIO = {
    ("f4", "p"): 1.654, ("f4", "m"): 1.000, ("f4", "v"): 1.323,
    ("f2", "p"): 1.603, ("f2", "m"): 1.000, ("f2", "v"): 1.303,
    ("odd", "p"): 1.306, ("odd", "m"): 1.000, ("odd", "v"): 1.281,
    ("offset", "p"): 1.224, ("offset", "m"): 1.000, ("offset", "v"): 1.323,
    ("sweep", "p"): 1.512, ("sweep", "m"): 1.000, ("sweep", "v"): 1.620,
    ("rider", "p"): 1.542, ("rider", "m"): 1.000, ("rider", "v"): 1.417,
    ("betas", "p"): 1.396, ("betas", "m"): 1.587, ("betas", "v"): 1.935,
    ("dense", "p"): 1.149, ("dense", "m"): 1.000, ("dense", "v"): 2.322,
    ("multi", "p"): 1.000, ("multi", "m"): 1.000, ("multi", "v"): 1.356,
}


def case_named(name):
    return CASES[CASE_IDS.index(name)]


def seed_of(case, salt=0):
    return (zlib.crc32(case.name.encode()) + 7919 * salt) % (1 << 31)


def lr_of(case, step):
    return LRS[0] if step <= case.T // 2 else LRS[1]


def geometry(case):
    """(elements per lane, lanes per row, rows per workgroup) of the catch-up kernel, restated: 512 lanes, lanes per row rounded
    up to 64.  tests/test_host_adam_routes.py holds this against the library's plan; the schedule's extra lists and the
    second-chunk defect model are built on it."""
    epl = 4 if case.D % 4 == 0 and case.off == 0 else 2
    lanes = (-(-case.D // epl) + 63) // 64 * 64
    rpb = 1
    while rpb < 16 and CATCH_THREADS // (rpb * 2) >= lanes:
        rpb *= 2
    return epl, CATCH_THREADS // rpb, rpb


# ---------------------------------------------------------------------------------------------- the visiting schedule

def scheduled_rows(case):
    """[(row, gap, phase)]: the row is listed at steps phase, phase + gap + 1, ... so that every later visit finds ``gap`` pending
    zero-gradient steps.  Row 0 and the table's last row are among them."""
    free = [0, case.N - 1] + [r for r in range(5, case.N - 1, 13) if not RANDOM_ZONE[0] <= r < RANDOM_ZONE[1]]
    out = []
    for gap in GAPS:
        for phase in ((1, 2, 3) if gap == 33 else (1, 2)):
            out.append((free[len(out)], gap, phase))
    return out


@functools.lru_cache(maxsize=None)
def schedule(case):
    """Per step t = 1 .. T (index t - 1): (ids [L] int64, extras).  ids: the scheduled rows of this step, four seeded random rows,
    -3 and N + 2 (both skipped by every kernel), rotated by t and filled up to L with duplicates of its own valid entries.  extras:
    id lists of one more catch-up behind this step's (a catch-up of a few rows between two steps)."""
    rs = np.random.RandomState(seed_of(case))
    rpb = geometry(case)[2]
    out = []
    for t in range(1, case.T + 1):
        ids = [r for r, gap, phase in scheduled_rows(case) if t >= phase and (t - phase) % (gap + 1) == 0]
        ids += list(rs.choice(np.arange(*RANDOM_ZONE), 4, replace=False))
        valid = list(ids)
        ids += [-3, case.N + 2]
        ids = ids[t % len(ids):] + ids[:t % len(ids)]
        assert len(ids) <= case.L - 3, (case.name, t, len(ids))
        k = 0
        while len(ids) < case.L:
            ids.insert((5 * k + 1) % len(ids), valid[(3 * k + t) % len(valid)])
            k += 1
        extras = []
        if t in EXTRA_STEPS:
            n = (1, rpb - 1, rpb + 1)[EXTRA_STEPS.index(t)]
            if n > 0:
                extras.append(np.arange(RANDOM_ZONE[0], RANDOM_ZONE[0] + n, dtype=np.int64))
        out.append((np.asarray(ids, dtype=np.int64), extras))
    return out


def valid_rows(case, ids):
    return np.unique(ids[(ids >= 0) & (ids < case.N)])


def own_split(case, ids, world=3, rank=1):
    """The id list as the ownership form takes it: (global ids, local ids).  The first half of the list becomes global ids this rank
    owns (row * world + rank), with an entry another rank owns behind every second one (it names a row the step does not list: it
    must be skipped); the second half, the negative id and the id past the table included, stays a list of shard indices."""
    half = len(ids) // 2
    listed = set(valid_rows(case, ids).tolist())
    foreign = [r for r in range(case.N) if r not in listed]
    glob, k = [], 0
    for i, r in enumerate(ids[:half]):
        if r < 0 or r >= case.N:
            continue
        glob.append(int(r) * world + rank)
        if i % 2:
            glob.append(foreign[(7 * k) % len(foreign)] * world + (rank + 1 + k % 2) % world)
            k += 1
    local = np.concatenate([ids[half:], np.asarray([r for r in ids[:half] if r < 0 or r >= case.N], dtype=np.int64)])
    return np.asarray(glob, dtype=np.int64), local


def sweep_window(case, rows, step):
    """Table rows of the moving window behind a listed catch-up of ``rows`` ids that brings them to ``step`` (adam_plan.h restated;
    held against the plan by tests/test_host_adam_routes.py)."""
    forced = -1 if case.sweep is None else int(case.sweep)
    n = 0
    if rows > 0 and step > 0:
        if forced > 0:
            n = -(-case.N // forced)
        elif forced < 0 and case.N >= 12 * rows:
            n = min(-(-case.N // 32), rows)
    start = ((step - 1) * n) % case.N if n else 0
    return (start + np.arange(n)) % case.N


def launches(case, form="plain", flush_at=()):
    """The launches of one run as (kind, step, ids): ("catch", upto, ids) | ("step", t, ids) | ("flush", upto, None).  The plain form
    steps with mkb_adam_rows_step; the advance form defers every step but the first, as mkb_amd.optim.Adam does."""
    out = []
    for t in range(1, case.T + 1):
        ids, extras = schedule(case)[t - 1]
        if t >= 2:
            out.append(("catch", t - 1, ids))
            out += [("catch", t - 1, e) for e in extras]
        if form == "plain" or t == 1:
            out.append(("step", t, ids))
        if t in flush_at:
            out.append(("flush", t, None))
    out.append(("flush", case.T, None))
    return out


def replay_counts(case, form):
    """What the replays of a run walk, from a model of ``last``: {(kind, zero-gradient steps replayed, with a gradient step in front)}
    over every row visit, and ``last`` after the run.  In the advance form a row's first pending step takes its gradient row."""
    last = np.zeros(case.N, dtype=np.int64)
    seen = set()
    for kind, step, ids in launches(case, form):
        if kind == "step":
            last[valid_rows(case, ids)] = step
            continue
        rows = np.arange(case.N) if ids is None else np.unique(np.concatenate([valid_rows(case, ids), sweep_window(case, len(ids), step)]))
        advance = form != "plain" and step >= 2
        for r in rows:
            if 0 < last[r] < step:
                pending = step - last[r]
                seen.add((kind, int(pending - 1 if advance else pending), advance))
            elif 0 < last[r]:
                seen.add((kind, 0, False))
        last[rows.astype(np.int64)] = step  # (the exchange stamps every valid row it visits, pending or not)
    return seen, last


# ---------------------------------------------------------------------------------------------- the stream

@functools.lru_cache(maxsize=8)
def initial(case):
    """The table [N, D], float32 on the host: |p| ~ 1 and ~ 0.01 in alternating groups of four rows."""
    g = torch.Generator(device="cpu").manual_seed(seed_of(case, 1))
    scale = torch.tensor([case.p_scales[(r // 4) % 2] for r in range(case.N)])
    return torch.randn(case.N, case.D, generator=g) * scale[:, None]


@functools.lru_cache(maxsize=8)
def gradients(case):
    """Per step: (rows, values [len(rows), D] float32).  Hand-made and independent of the parameters: row r has scale
    G_SCALES[r % 4], and an all-zero gradient at the steps t with (r + t) % 5 == 0."""
    out = []
    for t in range(1, case.T + 1):
        rows = valid_rows(case, schedule(case)[t - 1][0])
        g = torch.Generator(device="cpu").manual_seed(seed_of(case, 100 + t))
        vals = torch.randn(len(rows), case.D, generator=g)
        scale = torch.tensor([0.0 if (r + t) % 5 == 0 else G_SCALES[r % 4] for r in rows], dtype=torch.float32)
        out.append((rows, vals * scale[:, None]))
    return out


def rider_initial(case):
    g = torch.Generator(device="cpu").manual_seed(seed_of(case, 2))
    return torch.randn(case.rider, generator=g) * 0.5, torch.randn(case.rider, generator=g)


def rider_gradient(base, t):
    return base * np.float32(G_SCALES[t % 4])


# ---------------------------------------------------------------------------------------------- the float64 reference

def rule64(p, m, v, g, step, lr, betas, eps=EPS, consts_step=None, consts_lr=None, eps_inside=False, decay_v=True):
    """One Adam step restated in float64 -> (p, m, v), new tensors.  consts_step / consts_lr: the step whose bias corrections and
    rate are used (defect models); eps_inside: eps added before the bias correction (a defect model)."""
    b1, b2 = betas
    s = step if consts_step is None else consts_step
    lr = lr if consts_lr is None else consts_lr
    m = m + (1 - b1) * (g - m)
    v = (b2 * v if decay_v else v) + (1 - b2) * g * g
    bc1, bc2 = 1 - b1 ** s, 1 - b2 ** s
    denom = (v.sqrt() + eps) / bc2 ** 0.5 if eps_inside else v.sqrt() / bc2 ** 0.5 + eps
    return p - (lr / bc1) * m / denom, m, v


DEFECTS = ("skip-replay", "skip-v-decay", "prev-consts", "eps-inside", "defer-lr-next", "odd-last", "chunk2")
DEFECT_TEXT = {
    "skip-replay": "a replayed zero-gradient step skipped (each row's first)",
    "skip-v-decay": "that step's decay of v omitted",
    "prev-consts": "replayed steps take the previous step's constants",
    "eps-inside": "eps added before the bias correction",
    "defer-lr-next": "a step with a gradient takes the following step's rate",
    "odd-last": "the last element of an odd row left out of that replayed step",
    "chunk2": "the second chunk of a wide row left out of that replayed step",
}


def applies(case, defect):
    if defect == "odd-last":
        return case.D % 2 == 1
    if defect == "chunk2":
        epl, lanes, _ = geometry(case)
        return case.D > epl * lanes
    return True


def live_rows(case):
    """Rows some step lists: every other row is never touched (its bits stay, m = v = 0)."""
    return np.unique(np.concatenate([rows for rows, _ in gradients(case)]))


def _dense_grads(case, live, dtype):
    pos = {int(r): i for i, r in enumerate(live)}
    for rows, vals in gradients(case):
        g = torch.zeros(len(live), case.D, dtype=dtype)
        g[[pos[int(r)] for r in rows]] = vals.to(dtype)
        yield rows, g


def run64(case, defect=None):
    """The stream through the float64 rule over the live rows -> {"p", "m", "v"} [len(live), D] numpy float64."""
    live = live_rows(case)
    pos = {int(r): i for i, r in enumerate(live)}
    p = initial(case)[live].double()
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    had_gradient = np.zeros(len(live), dtype=bool)  # the row has taken a non-zero gradient: its zero-gradient steps move it
    hit = np.zeros(len(live), dtype=bool)           # the one-off defects have struck this row
    epl, lanes, _ = geometry(case)
    for t, (rows, g) in enumerate(_dense_grads(case, live, torch.float64), start=1):
        listed = np.zeros(len(live), dtype=bool)
        listed[[pos[int(r)] for r in rows]] = True
        kw = dict(eps_inside=defect == "eps-inside")
        if defect == "defer-lr-next":
            kw["consts_lr"] = lr_of(case, min(t + 1, case.T))
        np_, nm, nv = rule64(p, m, v, g, t, lr_of(case, t), case.betas, **kw)
        replayed = ~listed & had_gradient  # a zero-gradient step some later launch replays
        if defect == "prev-consts" and t >= 2:
            wp, wm, wv = rule64(p, m, v, g, t, lr_of(case, t), case.betas, consts_step=t - 1, consts_lr=lr_of(case, t - 1))
            sel = torch.as_tensor(replayed)[:, None]
            np_, nm, nv = torch.where(sel, wp, np_), torch.where(sel, wm, nm), torch.where(sel, wv, nv)
        strike = replayed & ~hit
        if defect in ("skip-replay", "skip-v-decay", "odd-last", "chunk2") and strike.any():
            hit |= strike
            sel = torch.zeros(len(live), case.D, dtype=torch.bool)
            if defect == "odd-last":
                sel[torch.as_tensor(strike), case.D - 1] = True
            elif defect == "chunk2":
                sel[torch.as_tensor(strike), epl * lanes: 2 * epl * lanes] = True
            else:
                sel[torch.as_tensor(strike)] = True
            if defect == "skip-v-decay":
                wp, wm, wv = rule64(p, m, v, g, t, lr_of(case, t), case.betas, decay_v=False)
            else:
                wp, wm, wv = p, m, v
            np_, nm, nv = torch.where(sel, wp, np_), torch.where(sel, wm, nm), torch.where(sel, wv, nv)
        p, m, v = np_, nm, nv
        had_gradient |= listed & (g.abs().sum(1) > 0).numpy()
    return {"p": p.numpy(), "m": m.numpy(), "v": v.numpy()}


def run_torch(case, dtype):
    """torch.optim.Adam on CPU tensors of ``dtype`` over the live rows -> {"p", "m", "v"} numpy float64."""
    live = live_rows(case)
    q = torch.nn.Parameter(initial(case)[live].to(dtype))
    opt = torch.optim.Adam([q], lr=LRS[0], betas=case.betas, eps=EPS)
    for t, (_, g) in enumerate(_dense_grads(case, live, dtype), start=1):
        opt.param_groups[0]["lr"] = lr_of(case, t)
        q.grad = g
        opt.step()
    st = opt.state[q]
    return {"p": q.detach().double().numpy(), "m": st["exp_avg"].double().numpy(), "v": st["exp_avg_sq"].double().numpy()}


def ulp32(x):
    return np.spacing(np.abs(x).astype(np.float32)).astype(np.float64)


def err_rows(yard, f64):
    """err_ref per row: the yardstick's largest deviation from float64 over the row, at least one float32 ulp of the row's largest
    float64 entry.  -> (err [rows], floored [rows])"""
    dev = np.abs(yard - f64).max(1)
    floor = ulp32(np.abs(f64).max(1))
    return np.maximum(dev, floor), dev < floor


Reference = collections.namedtuple("Reference", "live f64 err floored real")


@functools.lru_cache(maxsize=None)
def reference(case):
    """live: the rows some step lists; f64 / err / floored: per quantity, the float64 result [len(live), D], err_ref [len(live)] and
    where it is the one-ulp floor; real: rows that took a non-zero gradient (every other row holds its initial bits)."""
    live = live_rows(case)
    f64, yard = run64(case), run_torch(case, torch.float32)
    err, floored = {}, {}
    for q in QUANTITIES:
        err[q], floored[q] = err_rows(yard[q], f64[q])
    real = np.zeros(len(live), dtype=bool)
    pos = {int(r): i for i, r in enumerate(live)}
    for rows, vals in gradients(case):
        moved = (vals.abs().sum(1) > 0).numpy()
        real[[pos[int(r)] for r in rows[moved]]] = True
    return Reference(live, f64, err, floored, real)


def ratios(case, got):
    """got: {"p", "m", "v"} [len(live), D] (any float array) -> per quantity the largest deviation from float64 / err_ref over the
    rows."""
    ref = reference(case)
    return {q: float((np.abs(np.asarray(got[q], dtype=np.float64) - ref.f64[q]).max(1) / ref.err[q]).max()) for q in QUANTITIES}


def defect_move(case, defect):
    """-> (largest move / tolerance over the compared quantities, the quantity): how far the float64 defect model lies from the
    clean float64 result, in units of the device test's tolerance ERR_FACTOR x err_ref."""
    moved = run64(case, defect)
    ref = reference(case)
    best = (0.0, None)
    for q in QUANTITIES:
        r = float((np.abs(moved[q] - ref.f64[q]).max(1) / (ERR_FACTOR * ref.err[q])).max())
        best = max(best, (r, q))
    return best


# ---------------------------------------------------------------------------------------------- dense tensors

@functools.lru_cache(maxsize=2)
def dense_stream(n, seed=3):
    """(p0 [n], [gradient of step 1 .. DENSE_STEPS]): element i has |p| scale P_SCALES[(i // 4) % 2] and gradient scale G_SCALES[i % 4],
    zero at (i + t) % 5 == 0.  A shorter tensor takes a prefix: the rule is element-wise, so its results are a prefix, bit for bit."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    i = torch.arange(n)
    p0 = torch.randn(n, generator=g) * torch.tensor(P_SCALES)[(i // 4) % 2]
    grads = []
    for t in range(1, DENSE_STEPS + 1):
        scale = torch.tensor(G_SCALES)[i % 4] * ((i + t) % 5 != 0)
        grads.append(torch.randn(n, generator=g) * scale)
    return p0, grads


def dense_reference(p0, grads, first_step=1, betas=(0.9, 0.999), width=1024):
    """The float64 rule and torch.optim.Adam (float32, CPU) over flat tensors stepped from ``first_step`` on with the rate LRS[0];
    err_ref per ``width`` elements.  -> f64 {q: [n]}, err {q: [n]} (each element carries its block's err_ref)"""
    n = p0.numel()
    p, m, v = p0.double(), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    q = torch.nn.Parameter(p0.clone())
    opt = torch.optim.Adam([q], lr=LRS[0], betas=betas, eps=EPS)
    opt.state[q] = {"step": torch.tensor(float(first_step - 1)), "exp_avg": torch.zeros(n), "exp_avg_sq": torch.zeros(n)}
    for k, g in enumerate(grads):
        p, m, v = rule64(p, m, v, g.double(), first_step + k, LRS[0], betas)
        q.grad = g.clone()
        opt.step()
    f64 = {"p": p.numpy(), "m": m.numpy(), "v": v.numpy()}
    yard = {"p": q.detach().double().numpy(), "m": opt.state[q]["exp_avg"].double().numpy(), "v": opt.state[q]["exp_avg_sq"].double().numpy()}
    err = {}
    pad = (-n) % width
    for name in QUANTITIES:
        a = np.pad(yard[name], (0, pad)).reshape(-1, width)
        b = np.pad(f64[name], (0, pad)).reshape(-1, width)
        err[name] = np.repeat(err_rows(a, b)[0], width)[:n]
    return f64, err
