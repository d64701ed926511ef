"""Negative samplers whose candidate pool does not come from the reference's uniform draw: frequency-weighted, in-batch, or a
pool the caller made.  No reference counterpart to match bit for bit (``NegativeSampling`` has one and stays as it is).

The pooled training step asks a sampler for two things: a pool of ``2 * size`` entity ids and, per batch row, how often each pool
position occurs among the row's ``size`` negatives.  Where the pool comes from is the sampler's business:

``negatives_from_pool``       -- the per-row filter of a GIVEN pool on the device (``mkb_pool_filter``): a pool entry is kept for a
                                 row iff it is none of the row's known answers and not the row's own target; the kept entries fill
                                 the row's ``size`` slots cyclically, in pool order.  Exact membership; the pool may repeat ids.
``PoolNegativeSampling``      -- the base class: ``generate`` = ``self._pool(sample, mode)`` + ``negatives_from_pool``.  Subclass it
                                 with a ``_pool`` of your own (a teacher's top k, a type-constrained set, mined hard negatives).
``WeightedNegativeSampling``  -- pool entries drawn with probability proportional to ``weights ** power``, by default the entity's
                                 degree in the training triples to the power 0.75 (the word2vec / PBG / DGL-KE choice): Vose's
                                 alias table built once on the host, one ``mkb_pool_draw_alias`` launch per batch.
``InBatchNegativeSampling``   -- the pool is ``2 * size`` of the batch's own tails (heads for head-batch), taken cyclically from a
                                 random offset: a step then touches no entity row beyond those of the batch.

The returned LongTensor ``[B, size]`` carries ``._mkb_pool`` like ``NegativeSampling``'s, so ``FusedTrainStep``, ``PooledLossStep``
and ``model(sample, negatives, mode)`` take the pooled kernels.  A row whose filter leaves nothing gets zeros and is reported
lazily by ``check()`` (``compose.Pipeline`` calls it once an epoch): there is no host round trip per batch.

Not covered: the sharded steps (``mkb_amd.parallel``, ``mkb_amd.table_rows``) take ``NegativeSampling`` only, and nothing here
rides the row-lazy optimizer's catch-up launch -- the pool draw and the filter are launches of their own.
"""
import numpy as np
import torch

from .. import _hip
from ..utils.true_keys import true_keys
from .negative_sampling import PoolInfo

__all__ = ["negatives_from_pool", "PoolNegativeSampling", "WeightedNegativeSampling", "InBatchNegativeSampling", "alias_table"]

ACCEPT_ONE = 1 << 32  # accept[v] of a column that always keeps its own entity


def new_status(device):
    """The zeroed status pair ``mkb_pool_filter`` accumulates into: [code, smallest failing row]."""
    return torch.zeros(2, dtype=torch.int32, device=device)


def raise_status(status):
    """Raise ``RuntimeError`` for the first row whose filter emptied the pool in the calls that wrote ``status`` (synchronises);
    the pair is zeroed again first, so the sampler can be used on."""
    code, row = status.tolist()
    if code == 0:
        return
    status.zero_()
    if code == _hip.ERR_EMPTY:
        raise RuntimeError(f"row {row}: the filter removed the whole candidate pool (every pool entry is a known answer of the "
                           f"row's query or its own target)")
    raise RuntimeError(f"row {row}: pool filter status {code}")


def negatives_from_pool(sample, mode, pool, size, true_triples, n_entity, n_relation, status=None):
    """-> LongTensor ``[B, size]`` on ``sample``'s device: row ``i`` holds ``concat(f, f, ...)[:size]``, ``f`` = the entries of ``pool``
    (``[2 * size]`` int64 on that device, duplicates allowed) that are neither a known answer of row ``i``'s query in ``true_triples``
    nor its own target, in pool order.  ``true_triples``: None or empty = nothing is known (only the target is dropped).

    The result carries ``._mkb_pool`` (``PoolInfo``: pool, position map, multiplicities, touched rows) and ``._mkb_status``, the
    device pair [code, row] in which a row that kept nothing is recorded (``raise_status`` reads it; pass ``status`` to accumulate
    over calls).  Nothing here waits for the device."""
    mode_id = _hip.side_id(mode, "negatives replace")
    _hip.require_device(sample, pool)
    sample = _hip.contiguous(sample, torch.int64)
    pool = _hip.contiguous(pool, torch.int64)
    dev = sample.device
    B, K = sample.shape[0], int(size)
    if sample.dim() != 2 or sample.shape[1] != 3 or B < 1:
        raise ValueError("sample must be [B, 3] with B >= 1")
    if pool.device != dev or pool.dim() != 1 or pool.numel() != 2 * K:
        raise ValueError(f"pool must be [2 * size] = [{2 * K}] int64 on {dev}")
    keys = None
    if true_triples is not None and len(true_triples):
        keys = true_keys(true_triples, dev, n_entity, n_relation)[mode]
    if status is None:
        status = new_status(dev)
    neg = torch.empty((B, K), dtype=torch.int64, device=dev)
    pos = torch.empty((B, K), dtype=torch.int32, device=dev)
    cnt = torch.empty((B, 2 * K), dtype=torch.uint16, device=dev)
    touched = torch.empty(2 * K + 2 * B, dtype=torch.int64, device=dev)
    with _hip.on_device(dev):
        _hip.check(_hip.lib().mkb_pool_filter(_hip.ptr(sample), B, mode_id, n_entity, n_relation, _hip.ptr(pool), K, _hip.ptr(keys),
                                              0 if keys is None else keys.numel(), _hip.ptr(neg), _hip.ptr(pos), _hip.ptr(cnt),
                                              _hip.ptr(touched), _hip.ptr(status), _hip.stream_ptr()), "mkb_pool_filter")
    neg._mkb_pool = PoolInfo(pool, pos, cnt, K, mode_id, sample, touched)
    neg._mkb_status = status
    return neg


class PoolNegativeSampling:
    """Base class of the samplers that make a pool and have it filtered per row: subclass it and write
    ``_pool(self, sample, mode) -> LongTensor [2 * size]`` on ``sample``'s device (``sample`` is int64, contiguous, on a ROCm
    device; ``self.draws`` counts the pools made so far).  Constructor arguments as ``NegativeSampling``'s."""

    def __init__(self, size, train_triples, entities, relations, seed=42):
        if not 1 <= int(size) <= 1024:
            raise ValueError("size must be in [1, 1024]")
        self.size = int(size)
        self.n_entity, self.n_relation = len(entities), len(relations)
        self.train_triples = train_triples
        self.seed, self.draws = int(seed), 0
        self._status = {}  # device -> the status pair of every generate call there

    def _pool(self, sample, mode):
        raise NotImplementedError("a PoolNegativeSampling subclass makes its pool in _pool(sample, mode)")

    def generate(self, sample, mode):
        """-> LongTensor [B, size] on ``sample``'s device (a CPU ``sample`` is moved to the device and the negatives back)."""
        if mode not in ("head-batch", "tail-batch"):
            raise ValueError("mode must be 'head-batch' or 'tail-batch'")
        origin = sample.device
        if not sample.is_cuda:
            sample = sample.cuda()
        sample = _hip.contiguous(sample, torch.int64)
        if sample.dim() != 2 or sample.shape[1] != 3 or sample.shape[0] < 1:
            raise ValueError("sample must be [B, 3] with B >= 1")
        dev = sample.device
        status = self._status.get(dev)
        if status is None:
            status = self._status[dev] = new_status(dev)
        pool = self._pool(sample, mode)
        self.draws += 1
        neg = negatives_from_pool(sample, mode, pool, self.size, self.train_triples, self.n_entity, self.n_relation, status=status)
        if origin != dev:
            self.check()
            return neg.to(origin)
        return neg

    def check(self):
        """Raise ``RuntimeError`` naming the first row whose filter emptied the pool in the batches generated so far (synchronises)."""
        for status in self._status.values():
            raise_status(status)

    def get_state(self):
        return self.seed, self.draws

    def set_state(self, state):
        self.seed, self.draws = int(state[0]), int(state[1])


def _checked_weights(weights, power, train_triples, n_entity):
    """-> float64 [n_entity], the unnormalised probabilities ``weights ** power``."""
    if isinstance(weights, str):
        if weights == "uniform":
            return np.ones(n_entity, dtype=np.float64)
        if weights != "degree":
            raise ValueError(f"weights must be 'degree', 'uniform' or an array [n_entity], not {weights!r}")
        t = np.asarray(train_triples, dtype=np.int64).reshape(-1, 3)
        if len(t) and (t[:, [0, 2]].min() < 0 or t[:, [0, 2]].max() >= n_entity):
            raise ValueError("train_triples name an entity outside [0, n_entity)")
        w = (np.bincount(t[:, 0], minlength=n_entity) + np.bincount(t[:, 2], minlength=n_entity)).astype(np.float64)
    else:
        try:
            w = np.asarray(weights, dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError("weights must be 'degree', 'uniform' or an array [n_entity] of non-negative numbers") from None
        if w.shape != (n_entity,):
            raise ValueError(f"weights must have shape [n_entity] = [{n_entity}], not {list(w.shape)}")
    power = float(power)
    if not np.isfinite(power):
        raise ValueError("power must be finite")
    if not np.isfinite(w).all() or (w < 0).any():
        raise ValueError("weights must be finite and non-negative")
    p = np.where(w > 0, np.power(np.where(w > 0, w, 1.0), power), 0.0)  # (a weight of 0 stays 0 for every power)
    if not np.isfinite(p).all() or not p.sum() > 0:
        raise ValueError("weights ** power must be finite with a positive sum")
    return p


def alias_table(p):
    """Vose's alias method in float64 for unnormalised probabilities ``p`` [n] (non-negative, positive sum) ->
    ``(accept int64 [n] in [0, 2^32], alias int32 [n])``: column ``v`` yields ``v`` with probability ``accept[v] / 2^32``, else
    ``alias[v]``.  An entity of probability 0 has ``accept = 0`` and is nobody's alias, so it can never be drawn."""
    p = np.asarray(p, dtype=np.float64)
    n = len(p)
    scaled = p * (n / p.sum())
    prob = np.ones(n, dtype=np.float64)
    alias = np.arange(n, dtype=np.int64)
    order = np.argsort(-scaled, kind="stable")
    small = [int(v) for v in order if scaled[v] < 1.0]  # popped from the end: the smallest first
    large = [int(v) for v in order if scaled[v] >= 1.0]
    scaled = scaled.copy()
    while small and large:
        s, g = small.pop(), large.pop()
        prob[s], alias[s] = scaled[s], g
        scaled[g] = (scaled[g] + scaled[s]) - 1.0
        (small if scaled[g] < 1.0 else large).append(g)
    # what is left over, on either list, is 1 up to rounding: the column keeps its own entity
    accept = np.clip(np.floor(prob * float(ACCEPT_ONE) + 0.5), 0, ACCEPT_ONE).astype(np.int64)
    zero = p == 0
    if (accept[zero] != 0).any() or zero[alias[accept < ACCEPT_ONE]].any():
        raise ArithmeticError("alias table: an entity of weight 0 can be drawn")
    return accept, alias.astype(np.int32)


class WeightedNegativeSampling(PoolNegativeSampling):
    """Pool entries drawn independently with probability ``p_e`` proportional to ``weights_e ** power``.

    ``weights``: ``"degree"`` (occurrences of the entity as head or tail in ``train_triples``), ``"uniform"``, or an array
    ``[n_entity]`` of non-negative numbers with a positive sum; anything else raises ``ValueError``.  An entity of weight 0 is
    never drawn.  The alias table is built once on the host (Vose's method, float64; ``accept`` rounded to 32 fractional bits, so
    the drawn distribution is within ``n_entity * 2^-31`` of ``p``); a pool is one ``mkb_pool_draw_alias`` launch, counter based:
    ``(seed, draws)`` is the whole generator state."""

    def __init__(self, size, train_triples, entities, relations, seed=42, weights="degree", power=0.75):
        super().__init__(size, train_triples, entities, relations, seed)
        self.probabilities = _checked_weights(weights, power, train_triples, self.n_entity)
        self.probabilities /= self.probabilities.sum()
        self.accept, self.alias = alias_table(self.probabilities)
        self._tables = {}  # device -> (accept, alias) there

    def _pool(self, sample, mode, words=None):
        dev = sample.device
        tables = self._tables.get(dev)
        if tables is None:
            tables = self._tables[dev] = (torch.as_tensor(self.accept, device=dev), torch.as_tensor(self.alias, device=dev))
        pool = torch.empty(2 * self.size, dtype=torch.int64, device=dev)
        with _hip.on_device(dev):
            _hip.check(_hip.lib().mkb_pool_draw_alias(_hip.ptr(tables[0]), _hip.ptr(tables[1]), self.n_entity, self.size,
                                                      self.seed & 0xFFFFFFFFFFFFFFFF, self.draws, _hip.ptr(pool), _hip.ptr(words),
                                                      _hip.stream_ptr()), "mkb_pool_draw_alias")
        return pool


class InBatchNegativeSampling(PoolNegativeSampling):
    """The candidates of a tail-batch are the batch's own tails (of a head-batch, its heads): pool = ``side(sample[(o + arange(2 *
    size)) % B])`` with ``o = RandomState(seed).randint(B)`` drawn per call on the host.  When ``2 * size > B`` the pool wraps and
    repeats entities, which is legal.  Every row's own target is in the pool and is dropped by the filter like any known answer.

    The generator is the host's: ``get_state()`` is ``(seed, draws, numpy state)``."""

    def __init__(self, size, train_triples, entities, relations, seed=42):
        super().__init__(size, train_triples, entities, relations, seed)
        self._rs = np.random.RandomState(self.seed)
        self._steps = {}  # device -> arange(2 * size) there

    def _pool(self, sample, mode):
        dev, B = sample.device, sample.shape[0]
        steps = self._steps.get(dev)
        if steps is None:
            steps = self._steps[dev] = torch.arange(2 * self.size, dtype=torch.int64, device=dev)
        o, side = int(self._rs.randint(B)), sample[:, 0 if mode == "head-batch" else 2]
        if o + 2 * self.size <= B:  # no wrap: the same entries as one strided copy
            return side[o: o + 2 * self.size].contiguous()
        return side[(steps + o) % B]

    def get_state(self):
        return self.seed, self.draws, self._rs.get_state()

    def set_state(self, state):
        """``get_state()``'s triple; a pair ``(seed, 0)`` starts the generator afresh (the offsets drawn so far depend on the batch
        sizes met, which a pair does not hold)."""
        if len(state) == 2 and int(state[1]) != 0:
            raise ValueError("an in-batch sampler resumes from get_state()'s triple (seed, draws, numpy state)")
        super().set_state(state[:2])
        self._rs = np.random.RandomState(self.seed)
        if len(state) > 2:
            self._rs.set_state(state[2])
