"""The numpy restatement the pool-sampler tests compare against (include/mkb_hip.h, "pool samplers"): the per-row filter of a given
pool, the alias method's integer mapping, the distribution an alias table implies, and the fixtures both test files share.  CPU
only; the kernels are never compared with themselves."""
import numpy as np

HEAD, TAIL = 1, 2  # MKB_MODE_HEAD, MKB_MODE_TAIL
TWO32 = 1 << 32


def side_keys(triples, mode, N, R):
    """utils/true_keys.py's array of one side: (a * R + r) * N + x, ascending and unique; a = the fixed entity, x the varying one."""
    t = np.asarray(triples, dtype=np.int64).reshape(-1, 3)
    a, x = (t[:, 2], t[:, 0]) if mode == HEAD else (t[:, 0], t[:, 2])
    return np.unique((a * R + t[:, 1]) * N + x)


def known_answers(keys, fixed, r, N, R):
    """A_i as a sorted array: the keys of query (fixed, r) are one contiguous range."""
    if keys is None or len(keys) == 0 or not (0 <= fixed < N and 0 <= r < R):
        return np.zeros(0, dtype=np.int64)
    base = (int(fixed) * R + int(r)) * N
    lo, hi = np.searchsorted(keys, base), np.searchsorted(keys, base + N)
    return keys[lo:hi] - base


def filter_pool(sample, mode, N, R, pool, K, keys):
    """-> (neg [B, K] int64, pos [B, K] int32, cnt [B, 2K] uint16, touched [2K + 2B] int64, empty rows) of mkb_pool_filter."""
    sample, pool = np.asarray(sample, dtype=np.int64), np.asarray(pool, dtype=np.int64)
    B, P = len(sample), 2 * K
    assert pool.shape == (P,)
    neg, pos, cnt = np.zeros((B, K), np.int64), np.zeros((B, K), np.int32), np.zeros((B, P), np.uint16)
    empty = []
    for i, (h, r, t) in enumerate(sample):
        fixed, target = (t, h) if mode == HEAD else (h, t)
        keep = ~np.isin(pool, known_answers(keys, fixed, r, N, R)) & (pool != target)
        f = np.flatnonzero(keep)
        if len(f) == 0:
            empty.append(i)
            continue
        slots = f[np.arange(K) % len(f)]
        neg[i], pos[i] = pool[slots], slots
        cnt[i] = np.bincount(slots, minlength=P)
    touched = np.concatenate([pool, sample[:, 0], sample[:, 2]])
    return neg, pos, cnt, touched, empty


def alias_pick(column_word, u, accept, alias, N):
    """Entry of the alias draw from its two 32-bit words (uint32 arrays): the column is the accepted word under the rejection mask."""
    mask = 0
    while mask < N - 1:
        mask = (mask << 1) | 1
    v = (np.asarray(column_word, dtype=np.int64) & mask) if N > 1 else np.zeros(len(u), dtype=np.int64)
    assert (v < N).all()
    return np.where(np.asarray(u, dtype=np.int64) < accept[v], v, alias[v].astype(np.int64))


def uniform_columns(rs, n, N):
    """n columns uniform on [0, N) by masked rejection of 32-bit words from ``rs`` -> the accepted words."""
    mask = 0
    while mask < N - 1:
        mask = (mask << 1) | 1
    out = np.zeros(0, dtype=np.int64)
    while len(out) < n:
        w = rs.randint(0, TWO32, size=2 * n, dtype=np.int64)
        out = np.concatenate([out, w[(w & mask) < N]])
    return out[:n]


def implied_distribution(accept, alias):
    """q_e = (accept_e + sum_{j: alias_j = e} (2^32 - accept_j)) / (n 2^32), in float64 from exact integers."""
    n = len(accept)
    mass = [int(a) for a in accept]
    for j in range(n):
        mass[int(alias[j])] += TWO32 - int(accept[j])
    assert sum(mass) == n * TWO32
    return np.array([m / (n * TWO32) for m in mass], dtype=np.float64)


def skewed_weights(N, seed=0):
    """deg ** 0.75 of a Zipf-like degree sequence, in a shuffled order."""
    deg = np.floor(1000.0 / (1 + np.arange(N))) + 1
    return np.random.RandomState(seed).permutation(deg) ** 0.75


# ---- the filter's fixture: rows made on purpose (tests/test_gpu_pool_sampler.py lists them), then random rows ----------------------
def filter_fixture(N, R, B, K, mode, seed):
    """-> (sample [B, 3], pool [2K], triples [n, 3], safe): no row's filter empties the pool, because pool entry ``safe`` (= N - 2, at
    one position only) is no row's target and, in ``triples``, nobody's known answer -- so a pool of ``safe`` repeated empties no row
    either.  The rows made on purpose come first, as many of them as B holds; needs N >= 8 and R >= 3.
      row 0: its query has no key at all.            row 1: its only known answer is its own target.
      row 2: its known answers cover every pool entry but ``safe``: that one negative fills all K slots.
      row 3: its target stands at several pool positions (2K >= 4) and is a known answer as well.
      rows 4 / 5: the queries with the smallest and with the largest key of the side."""
    assert N >= 8 and R >= 3
    rs = np.random.RandomState(seed)
    P = 2 * K
    var, fix = (0, 2) if mode == HEAD else (2, 0)  # columns of the varying entity (the target) and of the fixed one
    safe = N - 2
    pool = rs.randint(2, N - 2, size=P).astype(np.int64)  # entities 0, 1 and N - 1 stay out of the pool
    if P >= 4:
        pool[[1, P // 2, P - 1]] = pool[0]
    pool[2 if P >= 4 else 1] = safe

    def triple(fixed, r, x):
        t = [0, r, 0]
        t[fix], t[var] = fixed, x
        return t

    special = [
        (triple(1, 1, 0), []),                                          # no key; the target 0 is not in the pool
        (triple(1, 2, 1), [1]),
        (triple(2, 1, 0), sorted(set(pool.tolist()) - {safe})),
        (triple(3, 1, int(pool[0])), [int(pool[0]), 0]),
        (triple(0, 0, 1), [0, 1]),                                      # keys 0 and 1: the smallest there are
        (triple(N - 1, R - 1, 0), [N - 1, 0]),                          # (N R - 1) N + N - 1: the largest there is
    ][:B]
    sample, triples = [], []
    for row, answers in special:
        sample.append(row)
        triples += [triple(row[fix], row[1], int(x)) for x in answers]
    while len(sample) < B:  # random rows on queries of their own: relation 0, fixed entity in [4, N - 1)
        fixed = int(rs.randint(4, N - 1))
        x, answers = int(rs.randint(N - 2)), rs.randint(N - 2, size=rs.randint(0, 6))
        sample.append(triple(fixed, 0, x))
        triples += [triple(fixed, 0, int(a)) for a in answers] + [triple(fixed, 0, x)]
    return np.asarray(sample, dtype=np.int64), pool, np.asarray(triples, dtype=np.int64).reshape(-1, 3), safe
