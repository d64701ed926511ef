"""Case table and torch CPU replica of the relation-prediction term (mkb_amd/csrc/rel_step.hip, losses.RelationPrediction,
model.score_relations).  Shared by tests/test_host_relation_prediction.py, tests/test_gpu_relation_prediction.py and
tools/relation_prediction_errors.py, which writes profiles/r28_relation_prediction_errors.txt.

The replica writes out the [B, R, De] score expression of each of the five models (the forms oracle/closed.py states, default
mode: q = query(h, r') against t), then

    row_i = logsumexp_j (S_ij / T) - S_{i, r_i} / T,   value = lambda sum_i w_i row_i / W,

and takes autograd.  In float64 it is the reference; in float32 on the same inputs it is the yardstick: ``err_ref`` of a quantity
is max |float32 - float64|, never below 4 float32 ulps of the quantity's largest magnitude, and the device is held to ERR_FACTOR
= 8 x err_ref (the project's factor, tests/util_onevsall.py).  A (case, quantity) whose honest ratio is measured above 8 on the
MI355X goes into MEASURED_RATIO at twice its ratio with its cause next to it, and is never allowed more than a quarter of one
typical term of the sum behind the quantity.  tools/relation_prediction_errors.py prints every ratio.

Kinks: |z| (TransE) and |sin z| (pRotatE) have a derivative that jumps by a whole term where the argument crosses zero; within
rounding of a kink float32 and float64 take different branches and no float32 implementation agrees with float64 -- a property
of the function.  As in tests/util_distance_all.py a case's seed is advanced until every pair term is more than KINK_ULPS float32
ulps of the largest argument off a kink; pRotatE draws from a quarter of the range on the larger shapes (one kink instead of seven).
"""
import collections
import math

import numpy as np
import torch

MODELS = ("TransE", "RotatE", "ComplEx", "DistMult", "pRotatE")
N = 50  # entities: few, so that they repeat within a batch
GAMMA = 6.0
MODULUS = 0.7
T, LAMBDA = 0.5, 0.25

# name, hidden, R, B.  hidden 4, 37 (no 16-byte rows), 130, 300 (more than 256 units per row: a second
# unit slice in both passes, blockIdx.y > 0); R 1 (the term is exactly 0), 3, 5 (less than the pair-major turn of 8 and the
# relation tile of 8), 37, 130 (more than one turn and tile, no multiple of either); B 1, 7, 37, 130 (with few relation tiles the
# relation-major pass cuts B = 37 into 5 slices of 8 rows and B = 130 into 17: more than one batch slice, the last one short and no
# multiple of the 4 rows it keeps in flight).
SHAPES = (("h4-r1-b1", 4, 1, 1), ("h4-r1-b7", 4, 1, 7), ("h4-r3-b7", 4, 3, 7), ("h37-r5-b37", 37, 5, 37), ("h130-r37-b7", 130, 37, 7),
          ("h37-r130-b37", 37, 130, 37), ("h4-r5-b130", 4, 5, 130), ("h300-r5-b7", 300, 5, 7), ("h130-r3-b130", 130, 3, 130),
          ("h37-r37-b130", 37, 37, 130), ("h300-r37-b37", 300, 37, 37), ("h4-r130-b1", 4, 130, 1))
CASES = [(model,) + shape for model in MODELS for shape in SHAPES]
CASE_IDS = [f"{c[0]}-{c[1]}" for c in CASES]
SMALLEST = ("h4-r3-b7", 4, 3, 7)
QUANTITIES = ("loss", "pos", "S", "dS", "g_ent", "g_rel", "g_mod")

ERR_FACTOR = 8.0
FLOOR_ULPS = 4.0
KINK_ULPS = 2.0
# (case id, quantity) -> (the device's error / err_ref, its cause) where the ratio was measured above 8 on the MI355X with no defect
# behind it (profiles/r28_relation_prediction_errors.txt has every case and quantity)
MEASURED_RATIO: dict = {}
LARGE = 100000  # pair terms per batch from which pRotatE's tables take a quarter of the range (module docstring)


def dims(model, hidden):
    """(entity_dim, relation_dim)."""
    return {"RotatE": (2 * hidden, hidden), "ComplEx": (2 * hidden, 2 * hidden)}.get(model, (hidden, hidden))


def phase_div(gamma, hidden):
    """The model's float32 embedding_range / pi (models/base.py: _constants)."""
    rng = float(np.float32((float(np.float32(gamma)) + 2.0) / hidden))
    return float(np.float32(rng / math.pi))


Problem = collections.namedtuple("Problem", "model name hidden R B gamma ent rel modulus sample weight")


def score_block(model, ent, rel, modulus, sample, gamma, kd):
    """[B, R] scores of every relation between h_i and t_i, the [B, R, De] expression written out; tensors of one dtype.
    -> (scores, (the pair terms' distance to a kink [B, R, units], the largest argument) or None)."""
    h, t = ent[sample[:, 0]][:, None], ent[sample[:, 2]][:, None]  # [B, 1, De]
    r = rel[None]                                                   # [1, R, Dr]
    if model == "TransE":
        z = (h + r) - t
        return gamma - z.abs().sum(-1), (z.detach().abs(), float(z.detach().abs().max()))
    if model == "DistMult":
        return ((h * r) * t).sum(-1), None
    if model == "pRotatE":
        z = (h / kd + r / kd) - t / kd
        s = torch.sin(z)
        return gamma - modulus.reshape(()) * s.abs().sum(-1), (s.detach().abs(), float(z.detach().abs().max()))
    d = ent.shape[1] // 2
    if model == "ComplEx":
        c, s = r[..., :d], r[..., d:]
    else:
        c, s = torch.cos(r / kd), torch.sin(r / kd)
    q_re, q_im = h[..., :d] * c - h[..., d:] * s, h[..., :d] * s + h[..., d:] * c
    if model == "ComplEx":
        return (q_re * t[..., :d] + q_im * t[..., d:]).sum(-1), None
    a, b = q_re - t[..., :d], q_im - t[..., d:]
    n2 = a * a + b * b
    off = n2 > 0  # the modulus with the norm's sub-gradient at the origin, 0: a coinciding pair is kept out of the square root
    return gamma - (torch.sqrt(torch.where(off, n2, torch.ones_like(n2))) * off.to(n2.dtype)).sum(-1), None


PREFILL = 1e-3


def prefill(pb):
    """What the three gradient buffers hold before the call (float32: g_ent, g_rel, g_modulus [1, 1])."""
    rs = np.random.RandomState(3)
    return [rs.uniform(-PREFILL, PREFILL, size=shape).astype(np.float32) for shape in (pb.ent.shape, pb.rel.shape, (1, 1))]


def seed_block(pb):
    """A random d loss / d block [B, R] for the backward of model.score_relations alone."""
    return np.random.RandomState(11).uniform(-1.0, 1.0, size=(pb.B, pb.R)).astype(np.float32)


def replica(pb, dtype, weighted=True, weight_sum=None, pre=None, temperature=T, lam=LAMBDA, dblock=None, tables=None):
    """Every quantity of the term in ``dtype`` -> dict of numpy arrays (QUANTITIES; g_mod None without a trained modulus).
    pre: what the gradient buffers held; the gradient is added to it, in ``dtype``.  dblock: instead of the term, the backward of
    the block alone with this d loss / d block (loss is then sum(dblock * S)).  tables: (ent, rel) in place of the problem's."""
    ent = torch.tensor(pb.ent if tables is None else tables[0], dtype=dtype, requires_grad=True)
    rel = torch.tensor(pb.rel if tables is None else tables[1], dtype=dtype, requires_grad=True)
    mod = torch.tensor([[pb.modulus]], dtype=dtype, requires_grad=True)
    sample = torch.as_tensor(pb.sample)
    S, _ = score_block(pb.model, ent, rel, mod, sample, pb.gamma, phase_div(pb.gamma, pb.hidden))
    S.retain_grad()
    rows = torch.arange(pb.B)
    if dblock is not None:
        value = (torch.tensor(dblock, dtype=dtype) * S).sum()
    else:
        w = torch.tensor(pb.weight, dtype=dtype) if weighted else torch.ones(pb.B, dtype=dtype)
        W = w.sum() if weight_sum is None else torch.tensor(weight_sum, dtype=dtype)
        row = torch.logsumexp(S / temperature, 1) - S[rows, sample[:, 1]] / temperature
        value = lam * (w * row).sum() / W
    value.backward()
    grads = [ent.grad, rel.grad, mod.grad]
    if pre is not None:
        grads = [None if g is None else torch.tensor(p, dtype=dtype) + g for p, g in zip(pre, grads)]
    out = {"loss": value, "pos": S[rows, sample[:, 1]], "S": S, "dS": S.grad, "g_ent": grads[0], "g_rel": grads[1],
           "g_mod": grads[2] if pb.model == "pRotatE" else None}
    return {k: None if v is None else v.detach().numpy() for k, v in out.items()}


def kink_clear(pb):
    """True if every pair term of the batch is KINK_ULPS float32 ulps of the largest argument off the kinks of its model's score."""
    with torch.no_grad():
        _, kinks = score_block(pb.model, torch.tensor(pb.ent, dtype=torch.float64), torch.tensor(pb.rel, dtype=torch.float64),
                               torch.tensor([[pb.modulus]], dtype=torch.float64), torch.as_tensor(pb.sample), pb.gamma,
                               phase_div(pb.gamma, pb.hidden))
    if kinks is None:
        return True
    dist, largest = kinks
    return dist.numel() == 0 or float(dist.min()) > KINK_ULPS * 2.0 ** -24 * largest


def _draw(model, name, hidden, R, B, seed, gamma):
    rs = np.random.RandomState(seed)
    rng = (gamma + 2.0) / hidden
    scale = rng * (4.0 if model == "RotatE" else 1.0)  # (RotatE: distances of a few units, so that gamma - sum spreads over the row)
    if model in ("ComplEx", "DistMult"):
        scale = rng = 1.0  # (products of three entries: at the embedding range every score is ~0 and the softmax is flat)
    quarter = 0.25 if model == "pRotatE" and B * R * hidden >= LARGE else 1.0
    de, dr = dims(model, hidden)
    ent = rs.uniform(-scale * quarter, scale * quarter, size=(N, de)).astype(np.float32)
    rel = rs.uniform(-rng * quarter, rng * quarter, size=(R, dr)).astype(np.float32)
    if model in ("ComplEx", "DistMult"):
        # a sum of `hidden` products of three entries of either sign: rms sqrt(hidden) a^3 for entries of rms a -> a few units
        ent *= np.float32(1.5 * hidden ** (-1.0 / 6.0))
        rel *= np.float32(1.5 * hidden ** (-1.0 / 6.0))
    sample = np.stack([rs.randint(N, size=B), rs.randint(R, size=B), rs.randint(N, size=B)], 1).astype(np.int64)
    if B >= 7:
        sample[0, 2] = sample[0, 0]             # a row with h == t
        sample[2, 2] = sample[1, 0]             # an entity that is a head in one row and a tail in another
        sample[4] = sample[3]                   # two identical rows
        sample[5, 1], sample[6, 1] = 0, R - 1   # the first and the last relation as targets
    weight = rs.uniform(0.5, 1.5, size=B).astype(np.float32)
    return Problem(model, name, hidden, R, B, gamma, ent, rel, MODULUS, sample, weight)


_problems = {}


def problem(case, gamma=GAMMA):
    """The seeded batch of a case (cached): the first seed whose pair terms all stay off the kinks (kink_clear)."""
    model, name, hidden, R, B = case
    key = (case, gamma)
    if key not in _problems:
        base = 1000 * CASES.index(case) if case in CASES else 77000
        for seed in range(base, base + 50):
            pb = _draw(model, name, hidden, R, B, seed, gamma)
            if kink_clear(pb):
                break
        else:
            raise AssertionError(f"no seed keeps {model}-{name} off the kinks")
        _problems[key] = pb
    return _problems[key]


def yardstick(f32, f64):
    yard = {}
    for q in QUANTITIES:
        if f64.get(q) is not None:
            err = float(np.abs(f32[q].astype(np.float64) - f64[q]).max())
            yard[q] = max(err, FLOOR_ULPS * 2.0 ** -24 * float(np.abs(f64[q]).max()))
    return yard


_expected = {}


def expected(pb, key=None, **kw):
    """(float64 replica, err_ref per quantity) of a problem; cached under ``key`` when given, never modified."""
    if key is None or key not in _expected:
        f64, f32 = replica(pb, torch.float64, **kw), replica(pb, torch.float32, **kw)
        res = (f64, yardstick(f32, f64))
        if key is None:
            return res
        _expected[key] = res
    return _expected[key]


def typical_term(pb, f64, quantity):
    """One typical term of the sum behind a quantity: a dropped or doubled unit, relation or batch row moves it by about this much.
    loss: one row's share; pos / S: rms(pair term) = rms score spread / sqrt(units); dS: the rms seed (each IS one term); the
    gradients: the rms seed times the rms derivative of a pair term with respect to an operand (<= 1 for the distance models, an
    operand product for the bilinear ones)."""
    rms = lambda a: float(np.sqrt((np.asarray(a, dtype=np.float64) ** 2).mean()))
    if quantity == "loss":
        return abs(float(f64["loss"])) / pb.B
    if quantity in ("pos", "S"):
        return rms(f64["S"] - (pb.gamma if pb.model in ("TransE", "RotatE", "pRotatE") else 0.0)) / pb.hidden
    if quantity == "dS":
        return rms(f64["dS"])
    if quantity == "g_mod":
        return rms(f64["dS"]) * 0.5
    operand = {"TransE": 1.0, "RotatE": 0.5, "pRotatE": 0.5 * pb.modulus}.get(pb.model, rms(pb.ent) * rms(pb.rel))
    return rms(f64["dS"]) * operand


def tolerance(pb, f64, yard, quantity, steps=1):
    factor = max(ERR_FACTOR, 2.0 * MEASURED_RATIO.get((f"{pb.model}-{pb.name}", quantity), (0.0,))[0])
    return steps * min(factor * yard[quantity], max(ERR_FACTOR * yard[quantity], 0.25 * typical_term(pb, f64, quantity)))


def ratios(got, f64, yard):
    """{quantity: device error / err_ref} for the quantities in ``got``."""
    out = {}
    for q, v in got.items():
        if v is not None and f64.get(q) is not None:
            err = float(np.abs(np.asarray(v, dtype=np.float64).reshape(f64[q].shape) - f64[q]).max())
            out[q] = err / yard[q] if yard[q] > 0 else (0.0 if err == 0 else float("inf"))
    return out


def check(pb, got, f64, yard, what, steps=1, show=True):
    """Print every ratio, then hold every quantity in ``got`` to its tolerance."""
    rs = ratios(got, f64, yard)
    if show:
        print(f"{pb.model}-{pb.name} {what}: " + " ".join(f"{q}={v:.2f}" for q, v in rs.items()))
    for q, v in got.items():
        if v is None or f64.get(q) is None:
            continue
        err = float(np.abs(np.asarray(v, dtype=np.float64).reshape(f64[q].shape) - f64[q]).max())
        tol = tolerance(pb, f64, yard, q, steps)
        assert err <= tol, f"{pb.model}-{pb.name} {what} {q}: error {err:.3e} > {tol:.3e} (ratio {rs[q]:.2f})"


# ---------------------------------------------------------------------------------------------------- the device's side
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


def term_of(temperature=T, lam=LAMBDA):
    from mkb_amd import losses

    return losses.RelationPrediction(lam, temperature)


def device_launch(pb, weighted=True, weight_sum=None, pre=None, temperature=T, lam=LAMBDA):
    """One ``term.launch`` (``mkb_rel_step``) on a fresh model -> {loss, pos, g_ent, g_rel, g_mod} as numpy."""
    m = device_model(pb, pre)
    term = term_of(temperature, lam)
    W = None if weight_sum is None else torch.tensor([weight_sum], dtype=torch.float32).cuda()
    value = term.launch(m, torch.as_tensor(pb.sample).cuda(), torch.tensor(pb.weight).cuda() if weighted else None, W)
    torch.cuda.synchronize()
    return dict(grads_of(m, pb), loss=value.cpu().numpy(), pos=term.positive_score.cpu().numpy())


def device_block(pb, weighted=True, weight_sum=None, temperature=T, lam=LAMBDA):
    """The explicit sequence's forward half -> {S, dS, loss, pos} as numpy (dS = lambda x the softmax's seeds)."""
    m = device_model(pb)
    term = term_of(temperature, lam)
    sample = torch.as_tensor(pb.sample).cuda()
    W = None if weight_sum is None else torch.tensor([weight_sum], dtype=torch.float32).cuda()
    with torch.no_grad():
        S = m.score_relations(sample)
        value, pos, seeds = term.block_seeds(m, sample, torch.tensor(pb.weight).cuda() if weighted else None, W)
    torch.cuda.synchronize()
    return {"S": S.cpu().numpy(), "dS": (seeds * term._scale(seeds.device)).cpu().numpy(), "loss": value.cpu().numpy(), "pos": pos.cpu().numpy()}
