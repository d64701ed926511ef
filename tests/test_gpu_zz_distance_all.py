"""-m gpu: the all-entity losses of TransE / RotatE / pRotatE (mkb_amd/csrc/score_all_dist.hip; fused.DistanceAllStep,
fused.distance_score_all) against the float64 replica of tests/util_distance_all.py, whose docstring has the case table, the
yardstick and the tolerance (FACTOR x the float32 error of torch's own evaluation of the same expression).

  step          every case of U.CASES x the three losses, random weights, all three gradient buffers pre-filled: loss,
                positive_score, g_ent, g_rel, g_modulus of DistanceAllStep, and S / dS through mkb_dist_all_score_fwd and the
                stand-alone loss call;
  forward       the block of mkb_dist_all_score_fwd is the block of mkb_rank_scores, bit for bit;
  determinism   two runs of each of the three step calls: the same bits in the loss and every gradient buffer; a pre-filled buffer
                ends as its content + the step's result in one rounded addition;
  edges         two rows of one query, h == t, a target that is no key, a query without keys, a relation row of zeros (the candidate
                that IS the query entity: an exactly zero difference in every dimension), scores of magnitude 300, a row whose every
                other column is filtered (loss and gradients exactly 0);
  unaligned     tables that start 4 bytes past a 16-byte boundary: the same results, through the C ABI;
  explicit      losses.OneVsAll()(fused.distance_score_all(...), ...) through autograd against the step;
  optimizers    two steps with optim.Adam(lazy_rows=True) and with optim.Adagrad against dense torch optimizers on the replica;
  pipeline      compose.Pipeline.learn routes RotatE + OneVsAll and TransE + KvsAll through DistanceAllStep.

Why the file is named to be collected LAST of the -m gpu suite.  tests/test_gpu_pool_routes.py::
test_prefill_dirty_memory_and_a_given_weight_sum[sp-h8-protate] depends on what ran in the process before it: the pooled pRotatE
backward adds into gradient rows with float atomics, the order two of them land in decides one rounding of a pre-filled element, and
that case sits at its bound (run alone it gives 8.47 x err_ref against a factor of 8 and fails, identically on the commit before
this file existed; behind the files that precede it in the suite it gives 6.5 - 6.8 x and passes).  Any GPU test file sorted in
front of it changes the device memory it finds; sorted here, this file changes nothing for any older test.
"""
import numpy as np
import pytest
import torch

import util_distance_all as U

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32)).view(np.int32)


def _held(tag, got, f64, yard, factor=1.0):
    """Print error / yardstick of every quantity in ``got`` -> the quantities past FACTOR."""
    bad = []
    for q, ratio in U.ratios(got, f64, yard).items():
        print(f"distance-all-error {tag} {q}: yardstick {yard[q]:.3e} ratio {ratio:.2f} factor {U.FACTOR[q]}")
        if not ratio <= factor * U.FACTOR[q]:
            bad.append((tag, q, ratio))
    return bad


@pytest.mark.parametrize("case", U.CASES, ids=U.CASE_IDS)
def test_step_against_float64(case):
    pb = U.problem(case)
    pre = U.prefill(pb)
    bad = []
    for loss in U.LOSSES:
        f64, yard = U.expected(pb, loss, key=case, pre=pre)
        got = U.device_step(pb, loss, pre=pre)
        got.update(U.device_block(pb, loss))
        assert all(np.isfinite(v).all() for v in got.values() if v is not None)
        bad += _held(f"step {U.CASE_IDS[U.CASES.index(case)]} {loss}", got, f64, yard)
    assert not bad, bad


@pytest.mark.parametrize("case", U.CASES, ids=U.CASE_IDS)
def test_forward_block_has_the_bits_of_the_evaluation(case):
    from mkb_amd import evaluation, fused

    pb = U.problem(case)
    m = U.device_model(pb)
    ents, rels = {i: i for i in range(pb.N)}, {i: i for i in range(U.R)}
    ev = evaluation.Evaluation(true_triples=pb.triples, entities=ents, relations=rels, batch_size=pb.B, device="cuda", num_workers=0)
    _, want = ev.ranks(m, pb.sample, pb.mode, with_scores=True)
    with torch.no_grad():
        got = fused.distance_score_all(m, torch.as_tensor(pb.sample).cuda(), pb.mode)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(got.cpu().numpy()), _bits(want.cpu().numpy()))


DETERMINISM = [c for c in U.CASES if c[2] in ("h37-n1030-b130", "tile64-n129-b37", "wide300-n129-b7")]


@pytest.mark.parametrize("case", DETERMINISM, ids=[f"{c[0]}-{c[1]}-{c[2]}" for c in DETERMINISM])
def test_two_runs_have_the_same_bits_and_prefilled_buffers_accumulate(case):
    pb = U.problem(case)
    pre = U.prefill(pb)
    for loss in U.LOSSES:  # the three step calls
        first, second = U.device_step(pb, loss), U.device_step(pb, loss)
        for q in first:
            if first[q] is not None:
                assert np.array_equal(_bits(first[q]), _bits(second[q])), (loss, q)
        # every gradient element takes the finished result in ONE rounded fp32 addition: the expectation is that addition, made here
        filled = U.device_step(pb, loss, pre=pre)
        for k, q in enumerate(("g_ent", "g_rel", "g_mod")):
            if first[q] is not None:
                assert np.array_equal(_bits(filled[q]), _bits(pre[k] + first[q])), (loss, q)
        assert np.array_equal(_bits(filled["loss"]), _bits(first["loss"]))


# ---------------------------------------------------------------------------------------------------------------- edges
EDGE_N, EDGE_HIDDEN, ZERO_REL = 129, 37, U.R - 1


def _edge_problem(model, mode, gamma=U.GAMMA):
    """Eight designed rows (tail-batch; head-batch mirrors them): 0 / 1 one query with two answers, 2 h == t, 3 a target that is no
    key of a query that has others, 4 a query without keys, 5 a query whose every other entity is a known answer, 6 the relation of
    zeros, 7 the relation of zeros again with the query entity itself as the target."""
    head = mode == "head-batch"
    for seed in range(50):
        pb = U._draw(model, mode, EDGE_HIDDEN, EDGE_N, 8, 9000 + seed, gamma)
        rel = pb.rel.copy()
        rel[ZERO_REL] = 0.0
        rows = [(3, 1, 10), (3, 1, 11), (20, 2, 20), (30, 3, 40), (50, 4, 60), (70, 0, 5), (80, ZERO_REL, 90), (81, ZERO_REL, 81)]
        triples = [rows[0], rows[1], rows[2], (30, 3, 41), (30, 3, 42), rows[6], rows[7]] + [(70, 0, j) for j in range(EDGE_N) if j != 5]
        if head:
            rows, triples = [(t, r, h) for h, r, t in rows], [(t, r, h) for h, r, t in triples]
        pb = pb._replace(rel=rel, sample=np.array(rows, dtype=np.int64), triples=sorted(set(triples)))
        if U.kink_clear(pb, allow_zero=True):
            return pb
    raise AssertionError("no seed keeps the edge batch off the kinks")


@pytest.mark.parametrize("mode", U.MODES)
@pytest.mark.parametrize("model", U.MODELS)
def test_edge_rows_against_float64(model, mode):
    pb = _edge_problem(model, mode)
    A = U.label_mask(pb.sample, pb.mode, pb.triples, pb.N)
    target = pb.sample[:, 0 if mode == "head-batch" else 2]
    assert A[0].sum() == 2 and (A[0] == A[1]).all() and not A[3, target[3]] and A[3].sum() == 2 and not A[4].any()
    assert A[5].sum() == pb.N - 1 and not A[5, target[5]]
    # the zero relation: the candidate equal to the query entity is an exactly zero difference in every dimension
    with torch.no_grad():
        _, kinks = U.score_block(model, torch.tensor(pb.ent), torch.tensor(pb.rel), torch.tensor([[pb.modulus]]), torch.as_tensor(pb.sample),
                                 mode, pb.gamma, U.phase_div(pb.gamma, pb.hidden))
    query_entity = pb.sample[:, 2 if mode == "head-batch" else 0]
    if kinks is not None:
        assert not kinks[0][6, query_entity[6]].any() and not kinks[0][7, query_entity[7]].any()
    pre = U.prefill(pb)
    bad = []
    for loss in U.LOSSES:
        f64, yard = U.expected(pb, loss, pre=pre)
        got = U.device_step(pb, loss, pre=pre)
        got.update(U.device_block(pb, loss))
        assert all(np.isfinite(v).all() for v in got.values() if v is not None)
        # (a pair of the zero relation that contributed anything but 0 would be off by a whole term, dS ~ 1e-3: far past the tolerance)
        bad += _held(f"edge {model} {mode} {loss}", got, f64, yard)
        if loss == "filtered":
            assert not got["dS"][5].any(), "a row that keeps its target alone has no gradient"
            assert (got["dS"][0][target[1]] == 0) and (got["dS"][1][target[0]] == 0), "two rows of one query filter each other's target"
    assert not bad, bad


@pytest.mark.parametrize("mode", U.MODES)
@pytest.mark.parametrize("model", U.MODELS)
def test_a_row_whose_every_other_column_is_filtered_is_exactly_zero(model, mode):
    pb = _edge_problem(model, mode)
    pb = pb._replace(sample=pb.sample[5:6].copy(), weight=pb.weight[5:6].copy(), B=1)
    got = U.device_step(pb, "filtered")
    assert got["loss"] == 0.0 and not got["g_ent"].any() and not got["g_rel"].any()
    assert got["g_mod"] is None or not got["g_mod"].any()


@pytest.mark.parametrize("mode", U.MODES)
@pytest.mark.parametrize("model", U.MODELS)
def test_scores_of_magnitude_300_stay_finite_and_within_tolerance(model, mode):
    """gamma = 300 and tables at a twentieth of the embedding range: every score of every row between +200 and +300, the direction in
    which exp(s / T) and softplus(s) overflow when they are not taken relative to the row maximum."""
    case = (model, mode, "h37-n129-b7", 37, 129, 7)
    pb = U.problem(case, gamma=300.0, shrink=0.05)
    bad = []
    for loss in U.LOSSES:
        f64, yard = U.expected(pb, loss)
        assert 200.0 < f64["S"].min() and 290.0 < f64["S"].max() <= 300.0
        got = U.device_step(pb, loss)
        got.update(U.device_block(pb, loss))
        assert all(np.isfinite(v).all() for v in got.values() if v is not None)
        bad += _held(f"extreme {model} {mode} {loss}", got, f64, yard)
    assert not bad, bad


UNALIGNED = [c for c in U.CASES if c[2] == "tile64-n129-b37" and c[1] == "tail-batch"]


@pytest.mark.parametrize("case", UNALIGNED, ids=[c[0] for c in UNALIGNED])
def test_tables_off_a_16_byte_boundary_give_the_same_step(case):
    """Both tables one float past an aligned address (rows the forward's register tile would take: it is left for the lane kernel,
    the backward passes load 4 bytes at a time anyway): mkb_dist_all_step answers MKB_OK and holds the tolerance."""
    from mkb_amd import _hip, fused

    pb = U.problem(case)
    f64, yard = U.expected(pb, "softmax", key=("plain", case))
    m = U.device_model(pb)
    shifted = []
    for p in (m.entity_embedding, m.relation_embedding):
        buf = torch.zeros(p.numel() + 64, dtype=torch.float32, device="cuda")
        off = (-buf.data_ptr() // 4) % 4 + 1  # a float index that is 4 bytes past a 16-byte boundary
        view = buf[off: off + p.numel()].view_as(p)
        view.copy_(p.detach())
        assert view.data_ptr() % 16 == 4
        shifted.append(view)
    gr = fused.grad_buffers(m)
    ws = fused._dist_workspace(m, pb.B)
    sample, w = torch.as_tensor(pb.sample).cuda(), torch.tensor(pb.weight).cuda()
    loss, pos = torch.empty(1, device="cuda"), torch.empty(pb.B, device="cuda")
    rc = _hip.lib().mkb_dist_all_step(m._tables(shifted[0], shifted[1]), gr, _hip.ptr(sample), _hip.ptr(w), pb.B, _hip.mode_id(pb.mode),
                                      U.SETTINGS["softmax"]["T"], None, _hip.ptr(loss), _hip.ptr(pos), _hip.ptr(ws), ws.numel(),
                                      _hip.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0
    got = dict(U.grads_of(m, pb), loss=loss.cpu().numpy()[0], pos=pos.cpu().numpy())
    assert not _held(f"unaligned {case[0]}", got, f64, yard)


# ---------------------------------------------------------------------------------------------------------------- glue
EXPLICIT = [c for c in U.CASES if c[2] in ("h37-n129-b7", "tile64-n129-b37")]


@pytest.mark.parametrize("case", EXPLICIT, ids=[f"{c[0]}-{c[1]}-{c[2]}" for c in EXPLICIT])
def test_explicit_route_equals_the_step(case):
    from mkb_amd import fused, losses

    pb = U.problem(case)
    f64, yard = U.expected(pb, "softmax", key=("plain", case))
    m = U.device_model(pb)
    sample, w = torch.as_tensor(pb.sample).cuda(), torch.tensor(pb.weight).cuda()
    target = sample[:, 0 if pb.mode == "head-batch" else 2].contiguous()
    value = losses.OneVsAll(U.SETTINGS["softmax"]["T"])(fused.distance_score_all(m, sample, pb.mode), target, w)
    value.backward()
    torch.cuda.synchronize()
    auto = dict(U.grads_of(m, pb), loss=value.detach().cpu().numpy())
    step = U.device_step(pb, "softmax")
    assert not _held(f"explicit {U.CASE_IDS[U.CASES.index(case)]}", auto, f64, yard)
    for q, v in auto.items():  # each within its tolerance of float64
        if v is not None:
            assert np.abs(v.astype(np.float64) - step[q].reshape(v.shape)).max() <= 2 * U.FACTOR[q] * yard[q], q


LAZY_SHAPE = ("lazy-n4100-b7", 8, 4100, 7)  # 4,096 rows or more: the tables the two optimizers step row-lazily / row-sparsely


def _dense_two_steps(pb, loss, dtype, make):
    ent, rel, mod = (torch.tensor(a, dtype=dtype) for a in (pb.ent, pb.rel, [[pb.modulus]]))
    params = [ent, rel] + ([mod] if pb.model == "pRotatE" else [])
    opt = make(params)
    for _ in range(2):
        now = pb._replace(ent=ent.numpy().copy(), rel=rel.numpy().copy(), modulus=float(mod))
        r = U.replica(now, loss, dtype)
        for p, q in zip(params, ("g_ent", "g_rel", "g_mod")):
            p.grad = torch.from_numpy(r[q]).to(dtype)
        opt.step()
    return {"g_ent": ent.numpy(), "g_rel": rel.numpy(), "g_mod": mod.numpy() if pb.model == "pRotatE" else None}


@pytest.mark.parametrize("which", ["adam-lazy", "adagrad"])
@pytest.mark.parametrize("model,mode,loss", [("RotatE", "tail-batch", "softmax"), ("TransE", "head-batch", "kvs"), ("pRotatE", "tail-batch", "filtered")])
def test_two_optimizer_steps_equal_dense_torch_steps_on_the_replica(model, mode, loss, which):
    """The tables after two steps (named g_ent / g_rel / g_mod below only to share FACTOR: a step is linear in the gradient up to the
    optimizer's own rounding, which the float32 yardstick takes with the dense torch optimizer)."""
    from mkb_amd import _links, fused, optim

    pb = U.problem((model, mode) + LAZY_SHAPE)
    lr = 0.01
    dense = (lambda ps: torch.optim.Adam(ps, lr=lr)) if which == "adam-lazy" else (lambda ps: torch.optim.Adagrad(ps, lr=lr))
    f64, f32 = _dense_two_steps(pb, loss, torch.float64, dense), _dense_two_steps(pb, loss, torch.float32, dense)
    yard = {q: max(float(np.abs(f32[q] - f64[q]).max()), U.FLOOR_ULPS * 2.0 ** -24 * float(np.abs(f64[q]).max())) for q in f64 if f64[q] is not None}
    m = U.device_model(pb)
    params = [p for p in m.parameters() if p.requires_grad]
    opt = optim.Adam(params, lr=lr, lazy_rows=True) if which == "adam-lazy" else optim.Adagrad(params, lr=lr)
    assert _links.owner(m.entity_embedding) is opt
    step = fused.DistanceAllStep(m, U.marker(loss, pb.triples))
    sample, w = torch.as_tensor(pb.sample).cuda(), torch.tensor(pb.weight).cuda()
    for _ in range(2):
        step(sample, w, mode)
        opt.step()
        opt.zero_grad()
    m.sync_parameters()
    torch.cuda.synchronize()
    got = {"g_ent": m.entity_embedding.detach().cpu().numpy(), "g_rel": m.relation_embedding.detach().cpu().numpy(),
           "g_mod": m.modulus.detach().cpu().numpy() if model == "pRotatE" else None}
    assert float(np.abs(got["g_ent"] - pb.ent).max()) > 0
    assert not _held(f"optimizer {which} {model} {mode} {loss}", got, f64, yard)


@pytest.mark.parametrize("model,which", [("RotatE", "softmax"), ("TransE", "kvs")])
def test_pipeline_routes_the_distance_models_through_the_step(monkeypatch, model, which):
    from mkb_amd import compose, datasets, fused, losses

    N, hidden, B = 131, 16, 32
    pb0 = U._draw(model, "tail-batch", hidden, N, 4 * B, 4242, U.GAMMA)
    rs = np.random.RandomState(5)
    # few heads and tails: most queries have several known answers
    train = sorted({(int(h), int(r), int(t)) for h, r, t in zip(rs.randint(12, size=8 * B), rs.randint(U.R, size=8 * B),
                                                                 rs.randint(N - 12, N, size=8 * B))})[: 4 * B]
    assert len(train) == 4 * B
    ents, rels = {i: i for i in range(N)}, {i: i for i in range(U.R)}
    ds = datasets.Dataset(train=train, batch_size=B, entities=ents, relations=rels, shuffle=False, num_workers=0, seed=42)
    m = U.device_model(pb0)

    class NoSampler:
        size = 16

        def generate(self, *args, **kwargs):
            raise AssertionError("the all-entity route draws no negatives")

    seen, inner = [], fused.DistanceAllStep.__call__

    def spy(self, sample, weight, mode, weight_sum=None):
        assert self.true_triples is ds.train
        out = inner(self, sample, weight, mode, weight_sum=weight_sum)
        seen.append((sample.cpu().numpy(), weight.cpu().numpy(), mode, float(out)))
        return out

    monkeypatch.setattr(fused.DistanceAllStep, "__call__", spy)
    opt = torch.optim.SGD([m.entity_embedding, m.relation_embedding], lr=0.0)  # the tables stay: every batch is the replica's
    pipe = compose.Pipeline(epochs=1, eval_every=100, device="cuda")
    pipe.device_batches = True
    marker = losses.OneVsAll(U.SETTINGS["softmax"]["T"]) if which == "softmax" else losses.KvsAll(label_smoothing=0.1)
    pipe.learn(model=m, dataset=ds, sampling=NoSampler(), optimizer=opt, loss=marker)
    assert len(seen) >= 4 and {s[2] for s in seen} == {"head-batch", "tail-batch"}
    for sample, weight, mode, got in seen:
        pb = pb0._replace(mode=mode, B=len(sample), sample=sample, weight=weight, triples=train)
        f64, yard = U.expected(pb, which)
        ratio = abs(got - float(f64["loss"])) / yard["loss"]
        print(f"distance-all-error pipeline {model} {mode} loss: yardstick {yard['loss']:.3e} ratio {ratio:.2f}")
        assert ratio <= U.FACTOR["loss"], (mode, got, float(f64["loss"]))
