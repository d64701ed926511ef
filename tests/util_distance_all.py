"""Case table and float64 replica of the all-entity losses of the distance models (mkb_amd/csrc/score_all_dist.hip,
fused.DistanceAllStep, fused.distance_score_all).  Shared by tests/test_host_distance_all.py, tests/test_gpu_zz_distance_all.py and
tools/distance_all_errors.py, which writes profiles/r26_distance_all_errors.txt.

The replica is torch on the CPU: it writes out the [B, N, De] expression of each model's score (oracle/closed.py states it) and takes
autograd through the loss formulas of losses/one_vs_all.py and losses/kvs_all.py.  Run in float64 it is the reference; run in float32
on the same inputs it is the yardstick: a quantity's tolerance is FACTOR x max(|float32 - float64|, 4 ulp of the quantity's largest
magnitude), FACTOR being twice the largest ratio the device showed over the whole case table on an MI355X, rounded up
(profiles/r26_distance_all_errors.txt has the table; the bits are deterministic, the factor 2 is head-room for a compiler change).

Inputs are kept off the score's kinks.  |z| (TransE) and |sin z| (pRotatE) have a derivative that jumps by a whole term where the
argument crosses zero: where an input sits within rounding of a kink, float32 and float64 evaluate different branches and no float32
implementation agrees with float64 there -- a property of the function, not of a kernel -- and the yardstick would grow by a whole
term and stop measuring anything.  So a case's seed is advanced until every pair term of the batch is more than KINK_ULPS float32
ulps of the largest argument away from a kink (exact zeros that a test builds on purpose excepted: there the derivative is DEFINED,
as 0).  pRotatE's argument spans (-3 pi, 3 pi) at the model's own embedding range, seven kinks, which a batch of millions of pair
terms cannot all avoid: the two large shapes draw pRotatE's tables from a quarter of the range (|z| < 3 pi / 4, the kink at 0 only);
the smaller shapes keep the whole range and with it every quadrant of the device's sine and cosine.
"""
import collections
import math

import numpy as np
import torch

MODELS = ("TransE", "RotatE", "pRotatE")
MODES = ("tail-batch", "head-batch")
R = 5
GAMMA = 6.0
MODULUS = 0.7

# name, hidden, N, B.  Every hidden in {4, 37, 130}, N in {9, 129, 1030} and B in {1, 7, 37, 130} of the issue appears, for every
# model and side; beyond them
#   tile64   rows the forward's register tile takes (TransE: entity_dim % 4 == 0 and >= 64, RotatE: hidden % 4 == 0 and >= 32): the
#            block then holds raw pair sums and the in-place finishing pass runs;
#   wide300  more than 256 units per row: a second unit slice in both backward passes (blockIdx.y > 0).
# The dQ pass splits the entities into several slices wherever N > 64 (N = 129: 3 slices of 64, N = 1030: 6 slices of 192); B = 130
# and N = 1030 are more than one staged block of 64 on the walked side, 37 / 129 / 1030 / 130 are no multiple of the 16-row tile.
SHAPES = (("h4-n9-b1", 4, 9, 1), ("h37-n129-b7", 37, 129, 7), ("h130-n1030-b37", 130, 1030, 37), ("h37-n1030-b130", 37, 1030, 130),
          ("tile64-n129-b37", 64, 129, 37), ("wide300-n129-b7", 300, 129, 7))
LOSSES = ("softmax", "filtered", "kvs")
SETTINGS = {"softmax": dict(T=0.5), "filtered": dict(T=0.5, eps=0.1), "kvs": dict(eps=0.1, reduction="mean")}
CASES = [(model, mode) + shape for model in MODELS for mode in MODES for shape in SHAPES]
CASE_IDS = [f"{c[0]}-{c[1]}-{c[2]}" for c in CASES]
QUANTITIES = ("loss", "pos", "S", "dS", "g_ent", "g_rel", "g_mod")

# twice the largest ratio measured over CASES x LOSSES on an MI355X, rounded up (profiles/r26_distance_all_errors.txt)
# measured: loss 3.05, pos 2.35, S 2.55, dS 2.05, g_ent 2.53, g_rel 1.86, g_mod 1.80
FACTOR = {"loss": 7, "pos": 5, "S": 6, "dS": 5, "g_ent": 6, "g_rel": 4, "g_mod": 4}
FLOOR_ULPS = 4.0
KINK_ULPS = 2.0  # (the arguments are sums of three rounded terms: their error stays below one ulp of the largest)


def entity_dim(model, hidden):
    return 2 * hidden if model == "RotatE" else hidden


def phase_div(gamma, hidden):
    """The model's float32 embedding_range / pi (models/base.py: _constants)."""
    rng = float(np.float32((float(np.float32(gamma)) + 2.0) / hidden))
    return float(np.float32(rng / math.pi))


Problem = collections.namedtuple("Problem", "model mode hidden N B gamma ent rel modulus sample weight triples")


def score_block(model, ent, rel, modulus, sample, mode, gamma, kd):
    """[B, N] scores of every entity in the open slot, the [B, N, De] expression written out; tensors of one dtype.
    -> (scores, (the pair terms' distance to a kink [B, N, units], the largest argument) or None)."""
    head = mode == "head-batch"
    h, r, t = ent[sample[:, 0]], rel[sample[:, 1]], ent[sample[:, 2]]
    x = ent[None]
    if model == "TransE":
        q = (r - t) if head else (h + r)
        z = (x + q[:, None]) if head else (q[:, None] - x)
        return gamma - z.abs().sum(-1), (z.detach().abs(), float(z.detach().abs().max()))
    if model == "pRotatE":
        q = (r / kd - t / kd) if head else (h / kd + r / kd)
        z = (x / kd + q[:, None]) if head else (q[:, None] - x / kd)
        s = torch.sin(z)
        return gamma - modulus.reshape(()) * s.abs().sum(-1), (s.detach().abs(), float(z.detach().abs().max()))
    d = ent.shape[1] // 2
    c, s = torch.cos(r / kd), torch.sin(r / kd)
    if head:
        q_re, q_im = c * t[:, :d] + s * t[:, d:], c * t[:, d:] - s * t[:, :d]
    else:
        q_re, q_im = h[:, :d] * c - h[:, d:] * s, h[:, :d] * s + h[:, d:] * c
    a, b = q_re[:, None] - x[..., :d], q_im[:, None] - x[..., d:]
    n2 = a * a + b * b
    off = n2 > 0  # the modulus with the norm's sub-gradient at the origin, 0: a coinciding pair is kept out of the square root
    return gamma - (torch.sqrt(torch.where(off, n2, torch.ones_like(n2))) * off.to(n2.dtype)).sum(-1), None


def label_mask(sample, mode, triples, N):
    """[B, N] bool: column j of row i is a known answer of row i's query in ``triples``."""
    head = mode == "head-batch"
    known = collections.defaultdict(set)
    for h, r, t in triples:
        known[(t, r) if head else (h, r)].add(h if head else t)
    mask = np.zeros((len(sample), N), dtype=bool)
    for i, (h, r, t) in enumerate(np.asarray(sample).tolist()):
        for j in known.get((t, r) if head else (h, r), ()):
            mask[i, j] = True
    return mask


PREFILL = 1e-3


def prefill(pb):
    """What the three gradient buffers hold before the step (float32: g_ent, g_rel, g_modulus [1, 1])."""
    rs = np.random.RandomState(3)
    return [rs.uniform(-PREFILL, PREFILL, size=shape).astype(np.float32) for shape in (pb.ent.shape, pb.rel.shape, (1, 1))]


def replica(pb, loss, dtype, settings=None, weight_sum=None, pre=None):
    """Every quantity of one step in ``dtype`` -> dict of numpy arrays (QUANTITIES; g_mod None without a trained modulus).  pre: what
    the gradient buffers held; the step's result is added to it, in ``dtype``."""
    st = dict(SETTINGS[loss] if settings is None else settings)
    ent = torch.tensor(pb.ent, dtype=dtype, requires_grad=True)
    rel = torch.tensor(pb.rel, dtype=dtype, requires_grad=True)
    mod = torch.tensor([[pb.modulus]], dtype=dtype, requires_grad=True)
    sample = torch.as_tensor(pb.sample)
    w = torch.ones(pb.B, dtype=dtype) if pb.weight is None else torch.tensor(pb.weight, dtype=dtype)
    W = w.sum() if weight_sum is None else torch.tensor(weight_sum, dtype=dtype)
    S, dist = score_block(pb.model, ent, rel, mod, sample, pb.mode, pb.gamma, phase_div(pb.gamma, pb.hidden))
    S.retain_grad()
    target = sample[:, 0 if pb.mode == "head-batch" else 2]
    rows = torch.arange(pb.B)
    A = torch.from_numpy(label_mask(pb.sample, pb.mode, pb.triples, pb.N))
    if loss == "kvs":
        y = (1.0 - st["eps"]) * A.to(dtype) + st["eps"] / pb.N
        c = 1.0 if st["reduction"] == "sum" else 1.0 / pb.N
        row = c * (torch.logaddexp(S, torch.zeros_like(S)) - y * S).sum(1)  # softplus without torch's cut at 20
    else:
        eps, T = st.get("eps", 0.0), st["T"]
        kept = torch.ones_like(A)
        if loss == "filtered":
            kept = ~A
            kept[rows, target] = True
        n = kept.sum(1, keepdim=True).to(dtype)
        y = (eps / n) * kept.to(dtype)
        y[rows, target] += 1.0 - eps
        z = torch.where(kept, S / T, torch.full_like(S, -float("inf")))
        row = torch.logsumexp(z, 1) - (y * torch.where(kept, S / T, torch.zeros_like(S))).sum(1)
    value = (w * row).sum() / W
    value.backward()
    grads = [ent.grad, rel.grad, mod.grad]
    if pre is not None:
        grads = [None if g is None else torch.tensor(p, dtype=dtype) + g for p, g in zip(pre, grads)]
    out = {"loss": value, "pos": S[rows, target], "S": S, "dS": S.grad, "g_ent": grads[0], "g_rel": grads[1],
           "g_mod": grads[2] if pb.model == "pRotatE" else None}
    return {k: None if v is None else v.detach().numpy() for k, v in out.items()}


def kink_clear(pb, allow_zero=False):
    """True if every pair term of the batch is KINK_ULPS float32 ulps of the largest argument off the kinks of its model's score
    (allow_zero: exact zeros aside, where a test builds them)."""
    with torch.no_grad():
        _, kinks = score_block(pb.model, torch.tensor(pb.ent, dtype=torch.float64), torch.tensor(pb.rel, dtype=torch.float64),
                               torch.tensor([[pb.modulus]], dtype=torch.float64), torch.as_tensor(pb.sample), pb.mode, pb.gamma,
                               phase_div(pb.gamma, pb.hidden))
    if kinks is None:
        return True
    dist, largest = kinks
    if allow_zero:
        dist = dist[dist != 0]
    return dist.numel() == 0 or float(dist.min()) > KINK_ULPS * 2.0 ** -24 * largest


LARGE = 1000000  # pair terms per batch from which pRotatE's tables take a quarter of the range (module docstring)


def _draw(model, mode, hidden, N, B, seed, gamma, shrink=1.0):
    """shrink: the tables' values as a fraction of the model's embedding range (of four times it for RotatE's entities)."""
    rs = np.random.RandomState(seed)
    rng = shrink * (gamma + 2.0) / hidden
    scale = rng * (4.0 if model == "RotatE" else 1.0)  # (RotatE: distances of a few units, so that gamma - sum spreads over the row)
    quarter = 0.25 if model == "pRotatE" and B * N * hidden >= LARGE else 1.0
    ent = rs.uniform(-scale * quarter, scale * quarter, size=(N, entity_dim(model, hidden))).astype(np.float32)
    rel = rs.uniform(-rng * quarter, rng * quarter, size=(R, hidden)).astype(np.float32)
    sample = np.stack([rs.randint(N, size=B), rs.randint(R, size=B), rs.randint(N, size=B)], 1).astype(np.int64)
    weight = rs.uniform(0.5, 1.5, size=B).astype(np.float32)
    # known triples: the batch's own, a second and third answer for most queries, some triples of queries that are not in the batch
    head = mode == "head-batch"
    triples = {tuple(s) for s in sample.tolist()}
    for h, r, t in sample.tolist():
        for _ in range(rs.randint(3)):
            o = int(rs.randint(N))
            triples.add((o, r, t) if head else (h, r, o))
    for _ in range(B):
        triples.add((int(rs.randint(N)), int(rs.randint(R)), int(rs.randint(N))))
    return Problem(model, mode, hidden, N, B, gamma, ent, rel, MODULUS, sample, weight, sorted(triples))


_problems = {}


def problem(case, gamma=GAMMA, shrink=1.0):
    """The seeded batch of a case (cached): the first seed whose pair terms all stay off the kinks (kink_clear)."""
    model, mode, name, hidden, N, B = case
    key = (case, gamma, shrink)
    if key not in _problems:
        base = 1000 * CASES.index(case) if case in CASES else 77000
        for seed in range(base, base + 50):
            pb = _draw(model, mode, hidden, N, B, seed, gamma, shrink)
            if kink_clear(pb):
                break
        else:
            raise AssertionError(f"no seed keeps {name} off the kinks")
        _problems[key] = pb
    return _problems[key]


_expected = {}


def expected(pb, loss, key=None, settings=None, weight_sum=None, pre=None):
    """(float64 replica, yardstick per quantity) of a problem; cached under ``key`` when given, never modified."""
    k = None if key is None else (key, loss)
    if k is None or k not in _expected:
        f64 = replica(pb, loss, torch.float64, settings, weight_sum, pre)
        f32 = replica(pb, loss, torch.float32, settings, weight_sum, pre)
        yard = {}
        for q in QUANTITIES:
            if f64[q] is not None:
                err = float(np.abs(f32[q].astype(np.float64) - f64[q]).max())
                yard[q] = max(err, FLOOR_ULPS * 2.0 ** -24 * float(np.abs(f64[q]).max()))
        if k is None:
            return f64, yard
        _expected[k] = (f64, yard)
    return _expected[k]


def ratios(got, f64, yard):
    """{quantity: device error / yardstick} for the quantities in ``got``."""
    out = {}
    for q, v in got.items():
        if v is not None and f64.get(q) is not None:
            err = float(np.abs(np.asarray(v, dtype=np.float64).reshape(f64[q].shape) - f64[q]).max())
            out[q] = err / yard[q] if yard[q] > 0 else (0.0 if err == 0 else float("inf"))
    return out


# ---------------------------------------------------------------------------------------------------- the device's side
def marker(loss, triples, settings=None):
    """The ``losses`` marker of a loss name at its SETTINGS."""
    from mkb_amd import losses

    st = dict(SETTINGS[loss] if settings is None else settings)
    if loss == "kvs":
        return losses.KvsAll(triples, st["eps"], st["reduction"])
    return losses.OneVsAll(st["T"], st.get("eps", 0.0), loss == "filtered", triples if loss == "filtered" else None)


def device_model(pb, pre=None):
    from util_gpu import make_model

    m = make_model(pb.model, pb.ent, pb.rel, pb.hidden, pb.gamma, modulus=[[pb.modulus]])
    if pre is not None:
        m.entity_embedding.grad, m.relation_embedding.grad = torch.tensor(pre[0]).cuda(), torch.tensor(pre[1]).cuda()
        if pb.model == "pRotatE":
            m.modulus.grad = torch.tensor(pre[2]).cuda()
    return m


def grads_of(m, pb):
    return {"g_ent": m.entity_embedding.grad.cpu().numpy(), "g_rel": m.relation_embedding.grad.cpu().numpy(),
            "g_mod": m.modulus.grad.cpu().numpy() if pb.model == "pRotatE" else None}


def device_step(pb, loss, settings=None, weight_sum=None, pre=None, weighted=True):
    """One ``fused.DistanceAllStep`` on a fresh model -> {loss, pos, g_ent, g_rel, g_mod} as numpy."""
    from mkb_amd import fused

    m = device_model(pb, pre)
    step = fused.DistanceAllStep(m, marker(loss, pb.triples, settings))
    W = None if weight_sum is None else torch.tensor([weight_sum], dtype=torch.float32).cuda()
    value = step(torch.as_tensor(pb.sample).cuda(), torch.tensor(pb.weight).cuda() if weighted else None, pb.mode, weight_sum=W)
    torch.cuda.synchronize()
    return dict(grads_of(m, pb), loss=value.cpu().numpy(), pos=step.positive_score.cpu().numpy()[:, 0])


def device_block(pb, loss, settings=None):
    """``mkb_dist_all_score_fwd`` and the stand-alone loss call on its block -> {S, dS} as numpy."""
    from mkb_amd import _hip, fused
    from mkb_amd.losses import kvs_all, one_vs_all
    from mkb_amd.utils.true_keys import true_keys

    st = dict(SETTINGS[loss] if settings is None else settings)
    m = device_model(pb)
    sample, w = torch.as_tensor(pb.sample).cuda(), torch.tensor(pb.weight).cuda()
    with torch.no_grad():
        S = fused.distance_score_all(m, sample, pb.mode)
    dS, mode_id = S.clone(), _hip.mode_id(pb.mode)
    keys = true_keys(pb.triples, S.device, pb.N, R)[pb.mode]
    if loss == "kvs":
        kvs_all.launch(dS, pb.N, sample, mode_id, R, keys, w, None, st["eps"], st["reduction"])
    elif loss == "filtered":
        one_vs_all.launch_filtered(dS, pb.N, sample[:, 0 if pb.mode == "head-batch" else 2].contiguous(), 1, sample, mode_id, R, keys, w, None,
                                   st["T"], st["eps"])
    else:
        one_vs_all.launch(dS, pb.N, sample[:, 0 if pb.mode == "head-batch" else 2].contiguous(), 1, w, None, st["T"])
    torch.cuda.synchronize()
    return {"S": S.cpu().numpy(), "dS": dS.cpu().numpy()}
