"""Test-only fp64 / Python restatement of a4r_mmr_rerank (include/a4r_diversify.h states the rule), a sim_lib-shaped stand-in for _lib.mmr_rerank
built on it, and the exact test data of tests/test_mmr_cpu.py / test_mmr_gpu.py.

The rule, restated once: entry j of a user's pool is valid iff 1 <= pid[j] < N1 and ps[j] is finite; r[j] = (ps[j] - smin) / (smax - smin) over the
valid entries, 1 when smax == smin; c(i, j) = <e_i, e_j> / (|e_i| |e_j|), 0 when either norm is 0; K greedy rounds, each taking the valid unselected
j with the largest v[j] = lam * r[j] - (1 - lam) * max over selected i of c(i, j) (0 while nothing is selected), ties to the smaller j; outputs the
picked pid / ps in pick order, id 0 / -inf in the slots left; ild = mean of 1 - c over the unordered pairs of picks, 0 with fewer than two."""
import numpy as np
import torch

MAX_POOL = 256


def mmr_user(emb64, pid, ps, lam, k):
    """One user.  emb64: float64 [N1, E]; pid, ps: the pool.  -> (ids int64 [k], scores float64 [k], ild, margins float64 [k], picks): margins[t] =
    best v - second-best v among the entries round t chose from (inf with fewer than two, or no round); picks = the pool positions, in order."""
    pid = np.asarray(pid, np.int64).reshape(-1)
    ps = np.asarray(ps, np.float64).reshape(-1)
    N1 = emb64.shape[0]
    valid = (pid >= 1) & (pid < N1) & np.isfinite(ps)
    ids = np.zeros(k, np.int64)
    out = np.full(k, -np.inf)
    margins = np.full(k, np.inf)
    pos = np.flatnonzero(valid)
    if pos.size == 0:
        return ids, out, 0.0, margins, []
    rows = emb64[pid[pos]]
    norm = np.sqrt((rows * rows).sum(1))
    s = ps[pos]
    lo, hi = s.min(), s.max()
    r = np.ones(pos.size) if hi == lo else (s - lo) / (hi - lo)
    m = np.full(pos.size, -np.inf)                                 # the largest cosine to a pick, once there is one
    free = np.ones(pos.size, bool)
    picks, pair_sum = [], 0.0
    for t in range(min(k, pos.size)):
        v = np.where(free, lam * r - (1.0 - lam) * (m if picks else 0.0), -np.inf)
        b = int(np.argmax(v))                                      # the first maximum: the smaller pool position
        rest = v[free & (np.arange(pos.size) != b)]
        if rest.size:
            margins[t] = v[b] - rest.max()
        den = norm[b] * norm
        c = np.where(den > 0, (rows @ rows[b]) / np.where(den > 0, den, 1.0), 0.0)
        pair_sum += float((1.0 - c[np.asarray(picks, np.int64)]).sum())                # the new pick against every pick before it
        picks.append(b)
        free[b] = False
        m = np.maximum(m, c)
        ids[t], out[t] = pid[pos[b]], ps[pos[b]]
    n = len(picks)
    return ids, out, (pair_sum / (n * (n - 1) / 2) if n >= 2 else 0.0), margins, [int(pos[b]) for b in picks]


def mmr_reference(item_emb, pool_ids, pool_scores, lam, k):
    """-> (ids int64 [U, k], scores float64 [U, k], ild float64 [U], margin float64 [U] = the smallest margin over the user's rounds,
    margins float64 [U, k] = every round's)."""
    emb64 = np.asarray(item_emb, np.float64)
    pool_ids, pool_scores = np.asarray(pool_ids), np.asarray(pool_scores)
    U = pool_ids.shape[0]
    ids, sc, ild, mg = np.zeros((U, k), np.int64), np.zeros((U, k)), np.zeros(U), np.zeros((U, k))
    for u in range(U):
        ids[u], sc[u], ild[u], mg[u], _ = mmr_user(emb64, pool_ids[u], pool_scores[u], lam, k)
    return ids, sc, ild, mg.min(1), mg


def sim_mmr_rerank(item_emb, pool_ids, pool_scores, lam, k, ids, scores, ild=None):
    """The simulated library's mmr_rerank: the restatement on the host."""
    assert pool_ids.dtype == torch.int32 and pool_scores.dtype == torch.float32 and pool_ids.shape == pool_scores.shape
    assert 1 <= k <= pool_ids.shape[1] <= MAX_POOL and 0.0 <= lam <= 1.0 and tuple(ids.shape) == (pool_ids.shape[0], k) == tuple(scores.shape)
    i, s, d, _, _ = mmr_reference(item_emb.cpu().numpy(), pool_ids.cpu().numpy(), pool_scores.cpu().numpy(), float(lam), int(k))
    ids.copy_(torch.from_numpy(i.astype(np.int32)))
    scores.copy_(torch.from_numpy(s.astype(np.float32)))
    if ild is not None:
        assert tuple(ild.shape) == (pool_ids.shape[0],) and ild.dtype == torch.float32
        ild.copy_(torch.from_numpy(d.astype(np.float32)))
    return ids, scores


# ------------------------------------------------------------------ exact data: every dot product, norm, cosine, relevance and v exact in fp32
ZERO_ROW = 7          # a row of zeros that is an item (norm 0: cosine 0 to everything)
TWINS = (3, 4)        # two items with the same row
LAMBDAS = (0.0, 0.25, 0.5, 1.0)


def exact_table(N1, E, seed=0):
    """fp32 [N1, E]: every row has exactly 64 non-zero entries, all +-2^k for one k per row (norm 8 * 2^k), drawn as sign flips of one of four base
    patterns so that cosines (multiples of 1/64) spread over [-1, 1]; row 0 (the pad item) and ZERO_ROW are zero, TWINS share a row and rows
    5, 6 are one row at two magnitudes (cosine 1)."""
    rng = np.random.default_rng(1000 + 7 * E + seed)
    t = np.zeros((N1, E), np.float32)
    bases = []
    for _ in range(4):
        b = np.zeros(E, np.float32)
        b[rng.permutation(E)[:64]] = rng.choice([-1.0, 1.0], size=64)
        bases.append(b)
    for i in range(1, N1):
        row = bases[int(rng.integers(0, 4))].copy()
        nz = np.flatnonzero(row)
        flip = nz[rng.permutation(64)[:int(rng.integers(0, 33))]]
        row[flip] = -row[flip]
        t[i] = row * np.float32(2.0 ** int(rng.integers(-2, 3)))
    if N1 > ZERO_ROW:
        t[ZERO_ROW] = 0
        t[TWINS[1]] = t[TWINS[0]]
        t[6] = t[5] * np.float32(4.0)
    return t


def exact_pool(U, P, N1, seed, special=True):
    """(pool_ids int32 [U, P], pool_scores fp32 [U, P]): integer scores whose range over each user's valid entries is a power of two (relevance is
    then k / 2^q); with ``special`` and room for them: pads (id 0 / -inf) at the tail and in the middle, a negative id and ids >= N1 with good
    scores, NaN / +inf / -inf scores on good ids, a repeated id, and (N1 > ZERO_ROW) the twins and the zero-norm row."""
    rng = np.random.default_rng(seed)
    pid = rng.integers(1, N1, size=(U, P)).astype(np.int64)
    ps = np.zeros((U, P), np.float64)
    for u in range(U):
        R = int(2 ** rng.integers(0, 6))
        base = int(rng.integers(-20, 20))
        ps[u] = base + rng.integers(0, R + 1, size=P)
        if special and P >= 15:
            if N1 > ZERO_ROW:
                pid[u, 0], pid[u, 1], pid[u, 4] = TWINS[0], TWINS[1], ZERO_ROW
            pid[u, 6] = pid[u, 2]                                  # a repeated id
            pid[u, 3], ps[u, 3] = 0, -np.inf                       # a pad in the middle
            pid[u, 5] = -3
            pid[u, 8] = N1
            pid[u, 9] = N1 + 12345
            ps[u, 10], ps[u, 11], ps[u, 12] = np.nan, np.inf, -np.inf
            pid[u, P - 2:], ps[u, P - 2:] = 0, -np.inf             # pads at the tail
        ok = np.flatnonzero((pid[u] >= 1) & (pid[u] < N1) & np.isfinite(ps[u]))
        if ok.size >= 2:                                           # both ends of the range are taken
            ps[u, ok[0]], ps[u, ok[-1]] = base + R, base
    return pid.astype(np.int32), ps.astype(np.float32)


GAUSSIAN_SEED = 3     # picked on the restatement alone so that at most 10 % of the users fall under tau: 0 % at E = 64, 7.8 % at E = 512 (where the share
                      # over seeds 1 .. 8 is 8 .. 17 %: the larger tau of the wider dot)


def gaussian_case(E, seed=GAUSSIAN_SEED, U=64, P=100, N1=4099):
    """The random case: a Gaussian table, distinct ids and uniform scores per pool."""
    rng = np.random.default_rng(seed)
    emb = rng.standard_normal((N1, E)).astype(np.float32)
    emb[0] = 0
    pid = np.stack([rng.permutation(N1 - 1)[:P] + 1 for _ in range(U)]).astype(np.int32)
    ps = rng.uniform(-1, 1, size=(U, P)).astype(np.float32)
    return emb, pid, ps


def tau(E):
    """The random case's decision threshold, 4 * (E + 16) * 2^-24: cosines are bounded by 1, an E-term fp32 dot carries at most about E * 2^-24 of
    error, 16 more ulps for the norms, the relevance and v, doubled because two values are compared, and doubled again."""
    return 4.0 * (E + 16) * 2.0 ** -24
