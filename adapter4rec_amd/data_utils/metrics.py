"""HR@10 / nDCG@10 evaluation with the reference's entry points (Downstream/Text/data_utils/metrics.py:62-116).

Same contract -- ``get_item_embeddings`` encodes all N+1 items with ``model.module.bert_encoder``; ``eval_model`` shards
users like ``SequentialDistributedSampler``, takes the last position of ``user_encoder``, scores against all items, masks
the history, drops the pad column and reports mean Hit@10 / nDCG@10 -- but the per-user Python loop, the [bs, N] fp64
label matrix and the argsort are replaced by one launch of a4r_eval_rank (rank of the target, history excluded, no
[users, items] matrix in HBM)."""
import math
import os

import numpy as np
import torch
import torch.distributed as dist

from .. import _lib as L
from .._lib_user_lists import LIST_MAX
from .._lib_diversify import MMR_MAX_POOL
from .dataset import SequentialDistributedSampler


def print_metrics(x, Log_file, v_or_t):
    Log_file.info(v_or_t + '_results   {}'.format('\t'.join(['{:0.5f}'.format(i * 100) for i in x])))


def _inner(model, args):
    m = model.module if hasattr(model, 'module') else model
    return m.model if 'compacter' in args.adapter_type and hasattr(m, 'model') else m


def get_item_embeddings(model, item_content, test_batch_size, args, use_modal, local_rank):
    """metrics.py:62-79 -> fp32 [N + 1, E] (on the device; the reference returns it on the CPU and moves it back)."""
    model.eval()
    inner = _inner(model, args)
    enc = inner.bert_encoder
    ed = getattr(args, 'eval_compute_dtype', None)
    if ed and ed != inner.compute_dtype:       # e.g. the item sweep in fp32 (the reference's eval precision) under bf16 training
        enc = inner.item_encoder_in(ed)
    dev = next(model.parameters()).device
    content = torch.as_tensor(np.asarray(item_content)).long()
    lo, hi, chunk, world = _my_shard(content.shape[0])
    out = []
    # the reference's test_batch_size (512 at run.py:650) is sized for ITS activation memory; the native encoder takes 4 096 titles per
    # call (fp32 sweep of 65 537 titles: 3.44 s at 512, 2.63 s = 84 % of the exact-fp32 MFMA peak at 4 096; profiles/r03_a_eval_bench.json)
    # A4R_EVAL_SWEEP_BATCH overrides it either way (e.g. a smaller sweep to fit memory next to a large training state).
    step = int(os.environ.get('A4R_EVAL_SWEEP_BATCH', 0)) or max(int(test_batch_size), 4096)
    with torch.no_grad():
        for i in range(lo, hi, step):
            out.append(enc(content[i:min(i + step, hi)].to(dev)))
    return _gather_shards(torch.cat(out, 0) if out else torch.zeros(0, enc_dim(model, args), device=dev), content.shape[0], chunk, world)


def enc_dim(model, args):
    return int(args.embedding_dim)


def _my_shard(n):
    """The item sweep is sharded over the data-parallel ranks (the reference encodes all N + 1 items on EVERY rank,
    metrics.py:62-79): rank r takes rows [r * chunk, (r + 1) * chunk) and the table is all-gathered."""
    world, r = _world_rank()
    chunk = (n + world - 1) // world
    return min(r * chunk, n), min((r + 1) * chunk, n), chunk, world


def _gather_shards(mine, n, chunk, world):
    if world == 1:
        return mine
    pad = torch.zeros(chunk, mine.shape[1], dtype=mine.dtype, device=mine.device)
    pad[:mine.shape[0]] = mine
    return _gather_cat(pad, world)[:n].contiguous()


def _world_rank():
    return (dist.get_world_size(), dist.get_rank()) if dist.is_initialized() else (1, 0)


def _shard_users(n_users, batch_size):
    """-> (world, rank, this rank's user ids): the run of consecutive users SequentialDistributedSampler hands the rank at this batch size, its
    tail repeating the last users.  eval_model and write_recommendations shard their users the same way."""
    world, rank = _world_rank()
    return world, rank, SequentialDistributedSampler(range(n_users), batch_size, rank=rank, num_replicas=world).indices()


def _gather_cat(t, world):
    """The ranks' equal-shaped tensors concatenated along dim 0 in rank order; ``t`` itself in a single process."""
    if world == 1:
        return t
    parts = [torch.zeros_like(t) for _ in range(world)]
    dist.all_gather(parts, t)
    return torch.cat(parts)


def _left_pad(flat, lens, width):
    """Rows of ``lens[i]`` item ids each, flattened in row order -> ids int64 / mask fp32 [n, width]: every row right-aligned, pad = width - len on
    the left (BuildEvalDataset.__getitem__'s layout), the mask 1 on the real positions."""
    n = lens.size
    rows = np.repeat(np.arange(n), lens)
    cols = (np.arange(int(lens.sum())) - np.repeat(np.cumsum(lens) - lens, lens)) + np.repeat(width - lens, lens)
    ids = np.zeros((n, width), dtype=np.int64)
    mask = np.zeros((n, width), dtype=np.float32)
    ids[rows, cols] = flat
    mask[rows, cols] = 1.0
    return ids, mask


def _csr_int32(rows):
    """A list of int64 id arrays as the kernels read per-user lists: (ptr int64 [n + 1], flat int32 ids + one spare 0, lens int64 [n])."""
    lens = np.fromiter((x.size for x in rows), dtype=np.int64, count=len(rows))
    ptr = np.zeros(len(rows) + 1, dtype=np.int64)
    np.cumsum(lens, out=ptr[1:])
    flat = np.concatenate(rows + [np.zeros(1, np.int64)])
    # ids outside int32 can never name a table row; clamp them to -1 (ignored like any id outside 1 .. N1-1) instead of letting them wrap
    flat = np.where((flat < 0) | (flat > np.iinfo(np.int32).max), -1, flat).astype(np.int32)
    return ptr, flat, lens


_PREP = {}        # (id(eval_seq), id(user_history), users, tokens, Lm, device) -> the evaluation set as device tensors (built once, reused every epoch)


def _prepare_eval_set(eval_seq, user_history, Lm, dev):
    """BuildEvalDataset.__getitem__ (data_utils/dataset.py:52-78) for ALL users at once, vectorised: left-padded input ids and log_mask [U, Lm - 1],
    the held-out target [U], and the histories as CSR (ptr [U + 1], flat ids) -- one pass over the two dicts instead of a Python loop per
    user and batch (round 5: 249 k users/s end to end against 4.4 M users/s for the rank kernel).  run.py hands the same two dicts to every
    evaluation of a run: the tensors are cached per (dict identities, sizes) and stay on the device."""
    import itertools
    n = len(eval_seq)
    key = (id(eval_seq), id(user_history), n, Lm, str(dev))
    hit = _PREP.get(key)
    if hit is not None and hit['_src'][0] is eval_seq and hit['_src'][1] is user_history:      # (the entry keeps both dicts alive: their ids cannot be re-used)
        return hit
    lens = np.fromiter((len(eval_seq[u]) for u in range(n)), dtype=np.int64, count=n)
    total = int(lens.sum())
    if n and int(lens.max()) > Lm:
        raise ValueError(f'an evaluation sequence of {int(lens.max())} items exceeds max_seq_len + 1 = {Lm}')
    flat = np.fromiter(itertools.chain.from_iterable(eval_seq[u] for u in range(n)), dtype=np.int64, count=total)
    ends = np.cumsum(lens)
    target = flat[ends - 1] if n else np.zeros(0, np.int64)
    keep = np.ones(total, dtype=bool)
    keep[ends - 1] = False                                    # every sequence's last item is the target, the rest its inputs
    ids, mask = _left_pad(flat[keep], lens - 1, Lm - 1)       # left padding: pad = Lm - len(seq)
    hv = [user_history[u] for u in range(n)]
    if n and isinstance(hv[0], torch.Tensor):                 # preprocess.py:58-59: one LongTensor per user
        hl = np.fromiter((t.shape[0] if t.dim() == 1 else t.numel() for t in hv), dtype=np.int64, count=n)
        hflat = (torch.cat(hv) if all(t.dim() == 1 for t in hv[:8]) else torch.cat([t.reshape(-1) for t in hv])).to(torch.int64)
    else:
        hl = np.fromiter((len(np.asarray(t).reshape(-1)) for t in hv), dtype=np.int64, count=n)
        hflat = torch.from_numpy(np.fromiter(itertools.chain.from_iterable(np.asarray(t).reshape(-1) for t in hv), dtype=np.int64, count=int(hl.sum())))
    if n and int(hl.max()) > L.EVAL_MAX_HISTORY:              # never truncate: an unmasked history item changes ranks silently
        u = int(hl.argmax())
        raise ValueError(f'user {u}: history of {int(hl.max())} items exceeds A4R_EVAL_MAX_HISTORY = {L.EVAL_MAX_HISTORY} '
                         f'(the reference keeps max_seq_len + 2 = {Lm + 1})')
    hptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(hl, out=hptr[1:])
    prep = dict(ids=torch.from_numpy(ids).to(dev), mask=torch.from_numpy(mask).to(dev), target=torch.from_numpy(target).to(dev),
                hptr=torch.from_numpy(hptr).to(dev), hptr_host=hptr, target32=torch.from_numpy(target.astype(np.int32)).to(dev),
                hflat32=torch.cat([hflat.to(torch.int32), torch.zeros(1, dtype=torch.int32)]).to(dev), _src=(eval_seq, user_history))
    if len(_PREP) >= 8:
        _PREP.clear()
    _PREP[key] = prep
    return prep


def _batch_slices(P, a, b):
    """The consecutive users a .. b - 1 of a prepared evaluation set as the kernels read them: (history ptr int32 [b - a + 1], counted from the
    batch's first id; the history ids; the targets int32 [b - a]) -- slices of the prepared tensors, no gather, no host-device round trip for
    the history count."""
    h0, h1 = int(P['hptr_host'][a]), int(P['hptr_host'][b])
    # (+ 1: the kernel's table is never empty; the store ends in one spare 0)
    return (P['hptr'][a:b + 1] - h0).to(torch.int32), P['hflat32'][h0:h1 + 1], P['target32'][a:b]


def candidate_mask(candidates, n1, dev):
    """A candidate set as a4r_eval_rank_cand / a4r_topk_items_cand read it: ``candidates`` (a bool or uint8 tensor, or an array, of N + 1 = n1
    entries; item i is a candidate iff entry i is non-zero, entry 0 -- the pad item -- is ignored) -> a uint8 tensor [n1] on ``dev``, uploaded
    here, once per call of the functions below.  None stays None (no restriction).  A wrong length, or no candidate among 1 .. N, raises
    ValueError."""
    if candidates is None:
        return None
    if isinstance(candidates, torch.Tensor):
        if candidates.dtype not in (torch.bool, torch.uint8):
            raise ValueError(f'candidates: a bool or uint8 tensor expected, got {candidates.dtype}')
        m = candidates
    else:
        m = torch.from_numpy(np.ascontiguousarray(np.asarray(candidates) != 0))
    if m.dim() != 1 or m.numel() != n1:
        raise ValueError(f'candidates: one entry per table row expected, [{n1}] (N + 1, entry 0 = the pad item), got {tuple(m.shape)}')
    if not bool((m[1:] != 0).any()):
        raise ValueError('candidates: no candidate among the items 1 .. N')
    m = m.to(dev).contiguous()
    return m.view(torch.uint8) if m.dtype == torch.bool else m


def read_candidates(path, item_names):
    """A candidate file -> bool array [N + 1]: one item name per line, the names --mode recommend writes (``item_names[i]`` = the item file's
    name of item i, [0] = the pad item: preprocess.read_behavior_names).  Blank lines and repeats are ignored; names that are no item raise
    ValueError listing the first few."""
    index = {name: i for i, name in enumerate(item_names) if i > 0 and name is not None}
    mask = np.zeros(len(item_names), dtype=bool)
    unknown = []
    with open(path) as f:
        for line in f:
            name = line.strip()
            if not name:
                continue
            i = index.get(name)
            if i is None:
                if name not in unknown:
                    unknown.append(name)
            else:
                mask[i] = True
    if unknown:
        raise ValueError(f'{path}: {len(unknown)} name(s) that are no item of this dataset: ' + ', '.join(unknown[:5]) + (' ...' if len(unknown) > 5 else ''))
    return mask


class Diversify:
    """recommend's ``diversify``: re-rank each user's ``pool`` best items by maximal marginal relevance (a4r_mmr_rerank; the rule is in
    include/a4r_diversify.h) -- k greedy picks by ``lam`` * relevance - (1 - ``lam``) * (largest cosine to an item already picked), relevance the
    score scaled to [0, 1] over the pool.  ``lam`` = 1 is the plain list; ``pool`` (at most MMR_MAX_POOL = 256) bounds how far down the ranking a
    pick can come from."""

    def __init__(self, lam=0.7, pool=100):
        self.lam, self.pool = float(lam), int(pool)
        if math.isnan(self.lam) or not 0.0 <= self.lam <= 1.0:
            raise ValueError(f'diversify: lambda = {self.lam} outside [0, 1]')
        if not 1 <= self.pool <= MMR_MAX_POOL:
            raise ValueError(f'diversify: pool = {self.pool} outside 1 .. {MMR_MAX_POOL}')


def _user_list(candidate_lists, u):
    """user u's entry of ``candidate_lists`` (a mapping, or a sequence indexed by user id), None where there is none"""
    if hasattr(candidate_lists, 'get'):
        return candidate_lists.get(u)
    return candidate_lists[u] if 0 <= u < len(candidate_lists) else None


def has_candidate_list(candidate_lists, uids):
    """bool [n]: whether each listed user has an entry in ``candidate_lists`` (an empty list is one)"""
    return np.fromiter((_user_list(candidate_lists, int(u)) is not None for u in uids), dtype=bool, count=len(uids))


def candidate_lists_csr(candidate_lists, uids):
    """The listed users' own candidate lists as a4r_topk_lists / a4r_eval_rank_lists read them: (ptr int64 [n + 1], flat int32 ids + one spare 0,
    lens int64 [n]), built on the host.  A user without an entry gets an empty list.  Ids outside int32 are clamped to -1 (ignored like any id
    outside 1 .. N).  A list longer than LIST_MAX raises ValueError naming the user: it is never truncated."""
    ls = []
    for u in uids:
        e = _user_list(candidate_lists, int(u))
        x = np.zeros(0, np.int64) if e is None else np.asarray(e if isinstance(e, (np.ndarray, torch.Tensor)) else list(e), dtype=np.int64).reshape(-1)
        if x.size > LIST_MAX:
            raise ValueError(f'user {int(u)}: candidate list of {x.size} items exceeds A4R_LIST_MAX = {LIST_MAX} (never truncated); '
                             'a catalogue-scale set belongs in a shared candidate set (--candidate_items)')
        ls.append(x)
    return _csr_int32(ls)


SCORE_DTYPES = ('fp32', 'bf16')


def _score_dtype_checked(score_dtype, **fp32_only):
    """``score_dtype`` validated; under 'bf16' every given restriction whose kernels are fp32-only is refused, not ignored."""
    if score_dtype not in SCORE_DTYPES:
        raise ValueError(f'score_dtype {score_dtype!r}, expected one of {SCORE_DTYPES}')
    if score_dtype == 'bf16':
        for name, value in fp32_only.items():
            if value is not None:
                raise ValueError(f"score_dtype 'bf16' cannot be combined with {name}: its kernels score in fp32 only")
    return score_dtype


def _cast_bf16(x):
    """The bf16 copy (round to nearest even, a4r_score_ce_bf16_cast) of a contiguous fp32 device tensor"""
    out = torch.empty(x.shape, dtype=torch.bfloat16, device=x.device)
    L.cast_bf16(x, out)
    return out


def _both_refused(candidates, candidate_lists, eval_negatives=None):
    if candidates is not None and candidate_lists is not None:
        raise ValueError('candidates (one set for all users) and candidate_lists (a list per user) cannot be combined: give one of them')
    if eval_negatives is not None and (candidates is not None or candidate_lists is not None):
        raise ValueError('eval_negatives (negatives drawn per user) cannot be combined with candidates or candidate_lists: give one of them')


def read_candidate_lists(path, user_names, item_names):
    """A candidate-list file -> {uid: [item ids]}: one line per user, ``user_name \\t item_name item_name ...`` with the names --mode recommend
    writes (``user_names[uid]``, ``item_names[i]`` with [0] = the pad item: preprocess.read_behavior_names).  Blank lines are ignored; a user
    named twice has the second line appended; a user named without items has an empty list.  Names that are no user or no item raise ValueError
    listing the first few."""
    users = {name: u for u, name in enumerate(user_names)}
    items = {name: i for i, name in enumerate(item_names) if i > 0 and name is not None}
    out, bad_users, bad_items = {}, [], []
    with open(path) as f:
        for line in f:
            if not line.strip():
                continue
            head, _, rest = line.rstrip('\n').partition('\t')
            u = users.get(head.strip())
            if u is None:
                if head.strip() not in bad_users:
                    bad_users.append(head.strip())
                continue
            ids = out.setdefault(u, [])
            for name in rest.split():
                i = items.get(name)
                if i is None:
                    if name not in bad_items:
                        bad_items.append(name)
                else:
                    ids.append(i)
    for bad, what in ((bad_users, 'user'), (bad_items, 'item')):
        if bad:
            raise ValueError(f'{path}: {len(bad)} name(s) that are no {what} of this dataset: ' + ', '.join(bad[:5]) + (' ...' if len(bad) > 5 else ''))
    return out


EVAL_NEG_SEED = 20240607          # --eval_neg_seed's default: one constant for every rank, epoch and run (a draw is keyed by the GLOBAL user id)


class EvalNegatives:
    """A sampled evaluation's spec: rank every target among ``n`` negatives drawn on the device from the items the user has not interacted with
    (include/a4r_eval_negatives.h: the draw rule, a pure function of seed, user id, the user's history and target, and the weights).
    ``counts`` None: uniform; else one occurrence count per table row ([N + 1], entry 0 -- the pad item -- ignored): an item is drawn in
    proportion to its count, an item of count 0 never.  Draws are independent: an id drawn twice counts once, so fewer than ``n`` distinct
    negatives may stand against a target.  The cumulative counts are built and uploaded once per (table size, device)."""

    def __init__(self, n, seed=EVAL_NEG_SEED, counts=None):
        self.n, self.seed = int(n), int(seed)
        if not 1 <= self.n <= LIST_MAX:
            raise ValueError(f'eval_negatives: n = {self.n} negatives outside 1 .. {LIST_MAX}')
        if not 0 <= self.seed < 2 ** 64:
            raise ValueError(f'eval_negatives: seed = {self.seed} outside 0 .. 2^64 - 1')
        self.counts = None
        if counts is not None:
            c = np.asarray(counts.cpu() if isinstance(counts, torch.Tensor) else counts).reshape(-1)
            if c.size < 2 or not np.issubdtype(c.dtype, np.integer) or (c[1:] < 0).any():
                raise ValueError('eval_negatives: counts must be non-negative integers, one per table row (entry 0 = the pad item)')
            self.counts = c.astype(np.int64)
            self.counts[0] = 0
        self._dev = {}
        self.last_err = None          # eval_ranks: the error word of its last evaluation (users without a candidate), a pinned int32 [1]

    def weights(self, n1, dev):
        """-> (cdf int64 [n1] on ``dev`` or None, cnt int64 [n1] on ``dev`` or None, whether some user could be left without a candidate)"""
        key = (int(n1), str(dev))
        if key not in self._dev:
            if self.counts is None:
                self._dev[key] = (None, None, n1 - 1 <= L.EVAL_MAX_HISTORY + 1)
            else:
                if self.counts.size != n1:
                    raise ValueError(f'eval_negatives: {self.counts.size} counts for a table of {n1} rows')
                cdf = np.cumsum(self.counts, dtype=np.int64)
                if float(self.counts.astype(np.float64).sum()) >= 2.0 ** 62:
                    raise ValueError('eval_negatives: the counts sum to 2^62 or more')
                top = np.sort(self.counts)[-(L.EVAL_MAX_HISTORY + 1):].sum()          # the most mass a history and a target can take out
                self._dev[key] = (torch.from_numpy(cdf).to(dev), torch.from_numpy(self.counts).to(dev), int(cdf[-1]) - int(top) < 1)
        return self._dev[key]


def item_counts(users_train, item_num):
    """--eval_neg_sampling pop: the occurrences of every item in the training sequences -> int64 [item_num + 1]"""
    import itertools
    flat = np.fromiter(itertools.chain.from_iterable(users_train.values()), dtype=np.int64)
    return np.bincount(flat[(flat > 0) & (flat <= item_num)], minlength=item_num + 1).astype(np.int64)


def _negatives_valid(spec, P, uid, n1, dev):
    """float [len(uid)]: 1 where the user has an item left to draw (m >= 1 in the draw rule).  Only a catalogue that a history can exhaust
    (uniform: at most 265 items; weighted: all but the 265 heaviest items weigh nothing) is looked at user by user, on the device."""
    _, cnt, possible = spec.weights(n1, dev)
    uid = torch.as_tensor(np.asarray(uid, dtype=np.int64)).to(dev)
    if not possible or uid.numel() == 0:
        return torch.ones(uid.numel(), device=dev)
    hp = P['hptr']
    lens = hp[uid + 1] - hp[uid]
    rows = torch.repeat_interleave(torch.arange(uid.numel(), device=dev), lens)
    within = torch.arange(int(lens.sum()), device=dev) - torch.repeat_interleave(torch.cumsum(lens, 0) - lens, lens)
    ids = torch.cat([P['hflat32'][hp[uid][rows] + within].long(), P['target'][uid].long()])
    rows = torch.cat([rows, torch.arange(uid.numel(), device=dev)])
    keep = (ids > 0) & (ids < n1)
    pairs = torch.unique(rows[keep] * n1 + ids[keep])
    w = torch.ones_like(pairs) if cnt is None else cnt[pairs % n1]
    mass = torch.zeros(uid.numel(), dtype=torch.int64, device=dev).scatter_add_(0, pairs // n1, w)
    total = n1 - 1 if cnt is None else int(cnt.sum().item())
    return (total - mass >= 1).float()


def write_eval_negatives(spec, user_history, eval_seq, n1, args, user_names, item_names, path, dev):
    """--eval_negatives_out: the materialised draws of every user of ``eval_seq`` (a4r_eval_draw_negatives: the ids a4r_eval_rank_sampled ranks
    against, bit for bit), one ``user_name \t item_name item_name ...`` line per user who has a candidate -- the --candidate_lists format, so the
    file given to --candidate_lists alone replays the evaluation of this split."""
    P = _prepare_eval_set(eval_seq, user_history, args.max_seq_len + 1, dev)
    cdf, _, _ = spec.weights(n1, dev)
    n_users = len(eval_seq)
    step = int(os.environ.get('A4R_EVAL_USER_BATCH', 0)) or 8192
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    written = 0
    with open(path, 'w') as f:
        for a in range(0, n_users, step):
            b = min(a + step, n_users)
            out = torch.zeros(b - a, spec.n, dtype=torch.int32, device=dev)
            ptr, hist, target = _batch_slices(P, a, b)
            L.eval_draw_negatives(ptr, hist, target, torch.arange(a, b, dtype=torch.int32, device=dev), cdf, spec.seed, n1, out, err)
            ids = out.cpu().numpy()
            for u in range(a, b):
                if ids[u - a, 0] != 0:                             # (no candidate: all zeros, no line -- the user is left out of the means either way)
                    f.write(user_names[u] + '\t' + ' '.join(item_names[int(i)] for i in ids[u - a]) + '\n')
                    written += 1
    if written + int(err.item()) != n_users:
        raise RuntimeError(f'eval negatives: {written} users drawn and {int(err.item())} counted without a candidate, of {n_users}')
    return written


def eval_ranks(model, user_history, eval_seq, item_embeddings, test_batch_size, args, user_ids, candidates=None, candidate_lists=None,
               eval_negatives=None, score_dtype='fp32'):
    """Rank (1 = best) of each listed user's held-out target among all items not in the user's history.  ``candidates`` (candidate_mask's
    input): among the candidate items only -- for every listed user; a target that is no candidate gets the rank it would have if it were.
    ``candidate_lists`` (a mapping, or a sequence indexed by user id, from user to an iterable of item ids, at most LIST_MAX each): among the
    user's own listed items only (a4r_eval_rank_lists: a sampled evaluation's negatives); a user without a list gets rank 1, the target need
    not be listed.  ``eval_negatives`` (an EvalNegatives): among the negatives drawn for the user on the device (a4r_eval_rank_sampled: one
    launch per batch draws, scores and ranks; the user's key is its id here, so the draws do not depend on the batch, the shard or the epoch); a
    user without a candidate gets rank 1 and is counted in ``eval_negatives.last_err``, a pinned word filled by an asynchronous copy: read it
    after the next synchronisation.  ``score_dtype`` 'bf16': the scores come from the bf16 MFMA at the rounded operands
    (a4r_eval_rank_bf16; the rule is in include/a4r_score_bf16.h) -- the table is cast once per call and each batch's user vectors once; the user
    tower still reads its input rows from the fp32 table, so the user vectors are the ones of 'fp32'.  Honoured with and without ``candidates``;
    refused beside ``candidate_lists`` and ``eval_negatives``, whose kernels score in fp32 only."""
    _both_refused(candidates, candidate_lists, eval_negatives)
    bf16 = _score_dtype_checked(score_dtype, candidate_lists=candidate_lists, eval_negatives=eval_negatives) == 'bf16'
    inner = _inner(model, args)
    dev = next(model.parameters()).device
    emb = item_embeddings.to(dev).float().contiguous()
    cand = candidate_mask(candidates, emb.shape[0], dev)
    Lm = args.max_seq_len + 1
    E = emb.shape[1]
    if len(user_ids) == 0:
        return torch.zeros(0, dtype=torch.int32, device=dev)
    P = _prepare_eval_set(eval_seq, user_history, Lm, dev)
    emb_b = _cast_bf16(emb) if bf16 else None                     # the scoring copy; the fp32 table stays: the user tower reads it
    uid_all = np.asarray(user_ids, dtype=np.int64)
    # (the sampler pads its tail by REPEATING the last user: a repeated id takes the rank of the entry before it)
    first = np.concatenate([[True], np.diff(uid_all) != 0])
    uid_np = uid_all[first]
    if candidate_lists is not None:                               # the CSR of the users' own lists, uploaded once, sliced per batch
        lptr, lflat_np, llens = candidate_lists_csr(candidate_lists, uid_np)
        lflat = torch.from_numpy(lflat_np).to(dev)
    if eval_negatives is not None:                                # the weights, uploaded once; one error word for the whole evaluation
        neg_cdf, _, _ = eval_negatives.weights(emb.shape[0], dev)
        neg_err = torch.zeros(1, dtype=torch.int32, device=dev)
    # SequentialDistributedSampler hands every rank a run of consecutive users (its tail repeats the last ones): a batch of CONSECUTIVE users is a
    # slice of every prepared tensor (_batch_slices)
    runs = np.flatnonzero(np.diff(uid_np) != 1) + 1
    bounds = np.concatenate([[0], runs, [uid_np.size]])
    # the reference's test_batch_size (256 - 512 users) is sized for ITS [users, items] score matrix; nothing of that size exists here: the user tower
    # and the rank kernel take 8 192 users per call (A4R_EVAL_USER_BATCH overrides it)
    step = int(os.environ.get('A4R_EVAL_USER_BATCH', 0)) or max(int(test_batch_size), 8192)
    ranks = []
    with torch.no_grad():
        for r0, r1 in zip(bounds[:-1], bounds[1:]):
            for s0 in range(int(r0), int(r1), step):
                a = int(uid_np[s0])
                nb = min(step, int(r1) - s0)
                b = a + nb
                input_embs = emb[P['ids'][a:b].reshape(-1)].view(nb, Lm - 1, E)
                prec = inner.user_encoder(input_embs, P['mask'][a:b], None)[:, -1].contiguous()
                ptr, hist, target = _batch_slices(P, a, b)
                rank = torch.zeros(nb, dtype=torch.int32, device=dev)
                if bf16:
                    L.eval_rank_bf16(_cast_bf16(prec), emb_b, target, ptr, hist, rank, cand)
                elif eval_negatives is not None:
                    L.eval_rank_sampled(prec, emb, target, ptr, hist, torch.arange(a, b, dtype=torch.int32, device=dev), neg_cdf,
                                        eval_negatives.seed, eval_negatives.n, rank, neg_err)
                elif candidate_lists is not None:
                    l0, l1 = int(lptr[s0]), int(lptr[s0 + nb])
                    L.eval_rank_lists(prec, emb, target, torch.from_numpy((lptr[s0:s0 + nb + 1] - l0).astype(np.int32)).to(dev),
                                      lflat[l0:l1 + 1], int(llens[s0:s0 + nb].max()), ptr, hist, rank)
                elif cand is None:
                    L.eval_rank(prec, emb, target, ptr, hist, rank)
                else:
                    L.eval_rank_cand(prec, emb, target, ptr, hist, cand, rank)
                ranks.append(rank)
    if eval_negatives is not None:                                # not waited for: the caller reads it after its own synchronisation
        host = torch.zeros(1, dtype=torch.int32)
        eval_negatives.last_err = (host.pin_memory() if dev.type == 'cuda' else host)
        eval_negatives.last_err.copy_(neg_err, non_blocking=True)
    out = torch.cat(ranks)
    if not first.all():
        out = out[torch.from_numpy(np.cumsum(first) - 1).to(dev)]
    return out


def eval_model(model, user_history, eval_seq, item_embeddings, test_batch_size, args, item_num, Log_file, v_or_t, local_rank, candidates=None,
               candidate_lists=None, eval_negatives=None, score_dtype='fp32'):
    """metrics.py:82-116.  Returns mean Hit@10 over all users (ranks are gathered over the data-parallel group).  ``candidates``
    (candidate_mask's input): every target is ranked among the candidate items only, and the means run over the users whose target is a
    candidate (cold-start and split evaluation); ValueError when there is no such user.  ``candidate_lists`` (eval_ranks'): every target is
    ranked among the user's own listed items, and the means run over the users who have a list; ValueError when no user has one.
    ``eval_negatives`` (an EvalNegatives): every target is ranked among the negatives drawn for its user on the device -- the sampled protocol of
    the SASRec / IDRec papers -- and the means run over the users who had an item left to draw.  ``score_dtype``: eval_ranks'."""
    _both_refused(candidates, candidate_lists, eval_negatives)
    _score_dtype_checked(score_dtype, candidate_lists=candidate_lists, eval_negatives=eval_negatives)
    n_users = len(eval_seq)
    world, _, user_ids = _shard_users(n_users, test_batch_size)
    model.eval()
    topK = 10
    dev = next(model.parameters()).device
    cand = candidate_mask(candidates, item_embeddings.shape[0], dev)          # uploaded once; eval_ranks takes it as it is
    Log_file.info(v_or_t + '_methods   {}'.format('\t'.join(['Hit{}'.format(topK), 'nDCG{}'.format(topK)])))
    ranks = eval_ranks(model, user_history, eval_seq, item_embeddings, test_batch_size, args, user_ids, candidates=cand,
                       candidate_lists=candidate_lists, eval_negatives=eval_negatives, score_dtype=score_dtype).float()
    valid, label, what = _validity(user_history, eval_seq, item_embeddings.shape[0], args, user_ids, dev, cand, candidate_lists, eval_negatives)
    hr = _means_over_valid(ranks, valid, n_users, topK, world, Log_file, v_or_t, label, what)
    if eval_negatives is not None and eval_negatives.last_err is not None:
        # the kernels' own count of the users without a candidate, read after the synchronisation of the means, must agree with the histories
        uid = np.asarray(user_ids, dtype=np.int64)
        first = torch.from_numpy(np.concatenate([[True], np.diff(uid) != 0])).to(dev) if uid.size else torch.zeros(0, dtype=torch.bool, device=dev)
        without = int((1.0 - valid)[first].sum().item())              # (the sampler's tail repeats the last user: counted once, as the kernel does)
        if int(eval_negatives.last_err.item()) != without:
            raise RuntimeError(f'{v_or_t}: the kernels counted {int(eval_negatives.last_err.item())} users without a candidate, the histories give {without}')
    return hr


def _validity(user_history, eval_seq, n1, args, user_ids, dev, cand, candidate_lists, eval_negatives):
    """Which of the listed users eval_model's means run over under each restriction -> (float flags [len(user_ids)], the label of the
    ``k of n users`` line, what a counted user has); (None, None, None) without a restriction: every user counts."""
    if eval_negatives is not None:                                    # the user has an item left to draw (computed from the histories)
        P = _prepare_eval_set(eval_seq, user_history, args.max_seq_len + 1, dev)
        return _negatives_valid(eval_negatives, P, user_ids, n1, dev), 'eval_negatives', 'has an item left to draw'
    if candidate_lists is not None:
        valid = torch.from_numpy(has_candidate_list(candidate_lists, user_ids).astype(np.float32)).to(dev)
        return valid, 'candidate_lists', 'has a candidate list'
    if cand is not None:
        P = _prepare_eval_set(eval_seq, user_history, args.max_seq_len + 1, dev)
        uid = torch.from_numpy(np.asarray(user_ids, dtype=np.int64)).to(dev)
        valid = (cand[P['target'][uid]] != 0).float() if uid.numel() else torch.zeros(0, device=dev)
        return valid, 'candidates', 'has a target among the candidate items'
    return None, None, None


def _means_over_valid(ranks, valid, n_users, topK, world, Log_file, v_or_t, label, what):
    """Hit@topK / nDCG@topK as means over the users whose validity flag is set (gathered over the data-parallel group beside hit and ndcg), the
    metrics line and ``<v_or_t>_<label>   k of n users``; ValueError when no user qualifies.  ``valid`` None (no restriction): the means over all
    users, and no such line."""
    hit = (ranks <= topK).float()
    ndcg = torch.where(ranks <= topK, 1.0 / torch.log2(ranks + 1.0), torch.zeros_like(ranks))
    if valid is None:             # the reference's fp32 .mean(), not sum / n_users: the two differ in the last bits, so this branch is not folded into the other
        hit, ndcg = _gather_cat(hit, world), _gather_cat(ndcg, world)
        mean_eval = [float(hit[:n_users].mean().item()), float(ndcg[:n_users].mean().item())]
        print_metrics(mean_eval, Log_file, v_or_t)
        return mean_eval[0]
    hit, ndcg, valid = (_gather_cat(t, world) for t in (hit * valid, ndcg * valid, valid))
    k = int(valid[:n_users].sum().item())
    if k == 0:
        raise ValueError(f'{v_or_t}: no user of {n_users} {what}')
    mean_eval = [float(hit[:n_users].sum().item()) / k, float(ndcg[:n_users].sum().item()) / k]
    print_metrics(mean_eval, Log_file, v_or_t)
    Log_file.info(v_or_t + '_{}   {} of {} users'.format(label, k, n_users))
    return mean_eval[0]


def _user_inputs(user_seqs, uids, T):
    """The user tower's input for the listed users: each one's last T items left-padded into ids / log_mask [n, T] (the layout _prepare_eval_set
    gives an evaluation input).  recommend and user_vectors build their inputs here."""
    import itertools
    seqs = [list(user_seqs[int(u)])[-T:] for u in uids]
    n = len(seqs)
    lens = np.fromiter((len(s) for s in seqs), dtype=np.int64, count=n)
    if n and int(lens.min()) == 0:
        raise ValueError(f'user {int(uids[int(lens.argmin())])}: an empty sequence has nothing to recommend from')
    return _left_pad(np.fromiter(itertools.chain.from_iterable(seqs), dtype=np.int64, count=int(lens.sum())), lens, T)


def _encode_users(inner, emb, ids_np, mask_np, a, b):
    """The user vectors of rows a .. b of _user_inputs' arrays: their items' rows of ``emb`` through user_encoder, last position -> fp32 [b - a, E]."""
    dev = emb.device
    x = torch.from_numpy(ids_np[a:b]).to(dev)
    input_embs = emb[x.reshape(-1)].view(b - a, ids_np.shape[1], emb.shape[1])
    return inner.user_encoder(input_embs, torch.from_numpy(mask_np[a:b]).to(dev), None)[:, -1].contiguous()


def _recommend_inputs(user_seqs, exclude, uids, T):
    """recommend()'s host side for the listed users: _user_inputs' ids / log_mask [n, T], and the exclusion lists as CSR (ptr [n + 1] int64,
    flat ids int32 + one spare 0)."""
    ids, mask = _user_inputs(user_seqs, uids, T)
    n = len(uids)
    ex =[np.asarray(exclude[int(u)]).reshape(-1).astype(np.int64) for u in uids] if exclude is not None else [np.asarray(user_seqs[int(u)], dtype=np.int64).reshape(-1) for u in uids]
    ptr, flat, el = _csr_int32(ex)
    if n and int(el.max()) > L.EVAL_MAX_HISTORY:              # never truncate: an unexcluded item would be recommended silently
        u = int(el.argmax())
        raise ValueError(f'user {int(uids[u])}: exclusion list of {int(el[u])} items exceeds A4R_EVAL_MAX_HISTORY = {L.EVAL_MAX_HISTORY}')
    return ids, mask, ptr, flat


def _id_array(x):
    """any iterable of item ids (a list, an array, a tensor, a set) -> int64 array [n]"""
    if isinstance(x, torch.Tensor):
        x = x.cpu().numpy()
    elif not isinstance(x, np.ndarray):
        x = list(x)
    return np.asarray(x, dtype=np.int64).reshape(-1)


def exclude_union_csr(base, exclude_lists, uids, n1):
    """The listed users' exclusion lists as a4r_topk_items_excl reads them: for each u of ``uids``, the union of ``base[u]`` and
    ``exclude_lists[u]`` (a user without an entry adds nothing), the ids outside 1 .. n1 - 1 dropped, ascending, each once -> (ptr int64 [n + 1],
    flat int32 ids + one spare 0), built on the host.  There is no cap on a list's length."""
    rows = []
    for u in uids:
        u = int(u)
        more = exclude_lists.get(u)
        x = _id_array(base[u])
        if more is not None:
            x = np.concatenate([x, _id_array(more)])
        rows.append(np.unique(x[(x >= 1) & (x < n1)]))
    ptr, flat, _ = _csr_int32(rows)
    return ptr, flat


def _exclude_lists_checked(exclude_lists, candidate_lists, score_dtype):
    """``exclude_lists`` beside what it cannot be combined with: refused, not ignored, before anything is encoded"""
    if exclude_lists is None:
        return
    if not hasattr(exclude_lists, 'get'):
        raise ValueError(f'exclude_lists: a dict {{uid: item ids}} expected, got {type(exclude_lists).__name__}')
    if candidate_lists is not None:
        raise ValueError('exclude_lists cannot be combined with candidate_lists: a shortlist is filtered where it is made')
    if score_dtype == 'bf16':
        raise ValueError("exclude_lists cannot be combined with score_dtype 'bf16': a4r_topk_items_excl scores in fp32 only")


def read_exclude_lists(path, user_names, item_names):
    """An exclusion-list file -> ({uid: [item ids]}, n_unknown_users, n_unknown_items): read_candidate_lists' line format, ``user_name \\t
    item_name item_name ...``; blank lines are ignored, a user named twice has the lines appended, a user named without items has an empty
    list.  Unlike a candidate list, a name that is no user or no item of this dataset is skipped and counted (distinct names), not raised: a
    block list and a user's old interactions legitimately name items that are no longer in the catalogue, and those cannot be recommended
    anyway."""
    users = {name: u for u, name in enumerate(user_names) if name is not None}
    items = {name: i for i, name in enumerate(item_names) if i > 0 and name is not None}
    out, bad_users, bad_items = {}, set(), set()
    with open(path) as f:
        for line in f:
            if not line.strip():
                continue
            head, _, rest = line.rstrip('\n').partition('\t')
            u = users.get(head.strip())
            if u is None:
                bad_users.add(head.strip())
                continue
            ids = out.setdefault(u, [])
            for name in rest.split():
                i = items.get(name)
                if i is None:
                    bad_items.add(name)
                else:
                    ids.append(i)
    return out, len(bad_users), len(bad_items)


def read_full_histories(behaviors_path, name2id, user_names, item_names):
    """The behaviours file itself as exclusion lists -> read_exclude_lists' triple: every item of a kept user's whole line (``user_name \\t
    item_name item_name ...``), not only the last max_seq_len + 3 that read_behaviors keeps.  ``name2id``: the item file's names (a name outside
    it is no item at all and is skipped uncounted, as read_behaviors skips it); a name of the item file that the reader dropped from the
    catalogue, and a user it dropped, are skipped and counted."""
    users = {name: u for u, name in enumerate(user_names) if name is not None}
    items = {name: i for i, name in enumerate(item_names) if i > 0 and name is not None}
    out, bad_users, bad_items = {}, set(), set()
    with open(behaviors_path) as f:
        for line in f:
            parts = line.strip('\n').split('\t')
            if len(parts) < 2 or not parts[0].strip():
                continue
            u = users.get(parts[0].strip())
            if u is None:
                bad_users.add(parts[0].strip())
                continue
            ids = out.setdefault(u, [])
            for name in parts[1].split():
                i = items.get(name)
                if i is not None:
                    ids.append(i)
                elif name in name2id:
                    bad_items.add(name)
    return out, len(bad_users), len(bad_items)


def merge_exclude_lists(*lists):
    """{uid: ids} dicts (None = none) -> one dict with each user's lists appended, or None when every one is None"""
    given = [x for x in lists if x is not None]
    if not given:
        return None
    out = {}
    for d in given:
        for u, ids in d.items():
            out.setdefault(u, []).extend(int(i) for i in ids)
    return out


def recommend(model, user_seqs, item_embeddings, k, args, exclude=None, user_ids=None, candidates=None, candidate_lists=None, diversify=None,
              score_dtype='fp32', exclude_lists=None):
    """The k best items for each listed user (default: every user of ``user_seqs``), after the user's sequence.

    ``user_seqs[u]``: the user's item ids (1 .. N); its last ``max_seq_len`` items go through ``user_encoder``, left-padded as an evaluation
    input is.  ``exclude[u]`` (default: ``user_seqs[u]``): items never returned, at most ``A4R_EVAL_MAX_HISTORY`` = 264 of them (longer lists
    raise ``ValueError``: never truncated); ids 0 or outside the table are ignored.  ``item_embeddings``: the fp32 [N + 1, E] table of
    ``get_item_embeddings`` / ``get_itemLMDB_embeddings`` / ``get_itemId_embeddings``.
    Returns (ids LongTensor [U, k], scores fp32 [U, k]) on the model's device: score descending, ties by smaller id; a user with fewer than k
    candidates gets id 0 / score -inf in the remaining slots.  One a4r_topk_items launch pair per batch of users (the [users, items] score matrix
    is never formed).  ``candidates`` (candidate_mask's input: bool / uint8 [N + 1], one set for all users): the lists are drawn from the
    candidate items only (a4r_topk_items_cand) -- the catalogue in stock, say, which no 264-id exclusion list could express.
    ``candidate_lists`` (eval_ranks': user -> an iterable of item ids, at most LIST_MAX each, longer lists raise ``ValueError``): the k best of
    the user's own listed items (a4r_topk_lists) -- a retrieval stage's shortlist, re-ranked; a user without a list gets pad slots only.
    ``diversify`` (a Diversify; k <= its pool): the entry above fills a pool of ``diversify.pool`` items per user instead, and a4r_mmr_rerank picks
    the k of them to return -- near-duplicates of an item already in the list give way to other items.  The scores are still the relevance
    scores, in pick order: they need not descend.
    ``score_dtype`` 'bf16': the scores come from the bf16 MFMA at the rounded operands (a4r_topk_items_bf16, include/a4r_score_bf16.h: the bits
    eval_ranks(score_dtype='bf16') compares) -- the table is cast once per call, each batch's user vectors once; the returned scores are those
    fp32 sums.  Honoured with and without ``candidates``; refused beside ``candidate_lists`` and ``diversify``, whose kernels score in fp32 only.
    ``exclude_lists`` ({uid: an iterable of item ids}, of any length; a user without an entry adds nothing): each user's list is added to what the
    user excludes already (``exclude[u]``, or ``user_seqs[u]``); the union goes sorted, each id once and without the ids outside 1 .. N, to
    a4r_topk_items_excl (include/a4r_exclude.h), which searches it in global memory -- every batch of the call goes through that entry, under
    ``candidates`` with its mask, and the 264-id cap does not apply (to ``exclude`` neither, then).  ``diversify`` composes: its pool is that
    entry's output.  Refused beside ``candidate_lists`` (a shortlist is filtered where it is made) and ``score_dtype`` 'bf16' (the entry scores in
    fp32 only).  None: nothing changes."""
    return _recommend(model, user_seqs, item_embeddings, k, args, exclude, user_ids, candidates, candidate_lists, diversify, False, score_dtype,
                      exclude_lists)[:2]


def _recommend(model, user_seqs, item_embeddings, k, args, exclude, user_ids, candidates, candidate_lists, diversify, want_ild, score_dtype='fp32',
               exclude_lists=None):
    """recommend's body -> (ids, scores, ild): ild None unless ``want_ild`` under ``diversify``, then fp32 [U, 2] = the intra-list diversity (mean
    1 - cosine over a list's pairs of items) of the plain top-k list and of the re-ranked one, both from the one pool."""
    _both_refused(candidates, candidate_lists)
    bf16 = _score_dtype_checked(score_dtype, candidate_lists=candidate_lists, diversify=diversify) == 'bf16'
    _exclude_lists_checked(exclude_lists, candidate_lists, score_dtype)
    if diversify is not None and not 1 <= int(k) <= diversify.pool:
        raise ValueError(f'diversify: k = {int(k)} outside 1 .. pool = {diversify.pool}')
    inner = _inner(model, args)
    dev = next(model.parameters()).device
    emb = item_embeddings.to(dev).float().contiguous()
    T = int(args.max_seq_len)
    k = int(k)
    cand = candidate_mask(candidates, emb.shape[0], dev)
    uids = np.arange(len(user_seqs), dtype=np.int64) if user_ids is None else np.asarray(user_ids, dtype=np.int64).reshape(-1)
    want_ild = want_ild and diversify is not None
    if uids.size == 0:
        return (torch.zeros(0, k, dtype=torch.long, device=dev), torch.zeros(0, k, dtype=torch.float32, device=dev),
                torch.zeros(0, 2, dtype=torch.float32, device=dev) if want_ild else None)
    kk = k if diversify is None else diversify.pool                # what the top-K entry is asked for
    if exclude_lists is None:
        ids_np, mask_np, ptr_np, flat_np = _recommend_inputs(user_seqs, exclude, uids, T)
    else:                                                          # the union as an int64-offset CSR, of any length: a4r_topk_items_excl's
        ids_np, mask_np = _user_inputs(user_seqs, uids, T)
        ptr_np, flat_np = exclude_union_csr(user_seqs if exclude is None else exclude, exclude_lists, uids, emb.shape[0])
        xptr = torch.from_numpy(ptr_np).to(dev)                    # uploaded once per call, sliced per batch
    step = int(os.environ.get('A4R_EVAL_USER_BATCH', 0)) or 8192          # (eval_ranks' user batch)
    flat = torch.from_numpy(flat_np).to(dev)
    emb_b = _cast_bf16(emb) if bf16 else None                     # the scoring copy; the fp32 table stays: the user tower reads it
    if candidate_lists is not None:                               # the CSR of the users' own lists, uploaded once, sliced per batch
        lptr, lflat_np, llens = candidate_lists_csr(candidate_lists, uids)
        lflat = torch.from_numpy(lflat_np).to(dev)
    out_ids, out_scores, out_ild = [], [], []
    model.eval()
    with torch.no_grad():
        for a in range(0, uids.size, step):
            b = min(a + step, uids.size)
            nb = b - a
            prec = _encode_users(inner, emb, ids_np, mask_np, a, b)
            h0, h1 = int(ptr_np[a]), int(ptr_np[b])
            ptr = torch.from_numpy((ptr_np[a:b + 1] - h0).astype(np.int32)).to(dev) if exclude_lists is None else None
            ids = torch.empty(nb, kk, dtype=torch.int32, device=dev)
            scores = torch.empty(nb, kk, dtype=torch.float32, device=dev)
            if exclude_lists is not None:                             # (the batch's offsets count from the whole array's start: a slice, no copy)
                L.topk_items_excl(prec, emb, xptr[a:b + 1], flat, cand, kk, ids, scores)
            elif bf16:
                L.topk_items_bf16(_cast_bf16(prec), emb_b, ptr, flat[h0:h1 + 1], kk, ids, scores, cand)
            elif candidate_lists is not None:
                l0, l1 = int(lptr[a]), int(lptr[b])
                L.topk_lists(prec, emb, torch.from_numpy((lptr[a:b + 1] - l0).astype(np.int32)).to(dev), lflat[l0:l1 + 1], int(llens[a:b].max()),
                             ptr, flat[h0:h1 + 1], kk, ids, scores)
            elif cand is None:
                L.topk_items(prec, emb, ptr, flat[h0:h1 + 1], kk, ids, scores)
            else:
                L.topk_items_cand(prec, emb, ptr, flat[h0:h1 + 1], cand, kk, ids, scores)
            if diversify is not None:                                 # ids / scores are the pool: cut it to k
                pool_ids, pool_scores = ids, scores
                ids = torch.empty(nb, k, dtype=torch.int32, device=dev)
                scores = torch.empty(nb, k, dtype=torch.float32, device=dev)
                ild = torch.empty(2, nb, dtype=torch.float32, device=dev) if want_ild else None                      # the plain list's, the re-ranked one's
                if want_ild:                                          # lambda = 1: the plain top-k list, for its diversity alone
                    L.mmr_rerank(emb, pool_ids, pool_scores, 1.0, k, ids, scores, ild[0])
                L.mmr_rerank(emb, pool_ids, pool_scores, diversify.lam, k, ids, scores, ild[1] if want_ild else None)
                if want_ild:
                    out_ild.append(ild.t())
            out_ids.append(ids.long())
            out_scores.append(scores)
    return torch.cat(out_ids), torch.cat(out_scores), (torch.cat(out_ild).contiguous() if want_ild else None)


def write_recommendations(model, user_seqs, user_history, item_embeddings, k, batch_size, args, user_names, item_names, path, candidates=None,
                          candidate_lists=None, diversify=None, Log_file=None, score_dtype='fp32', exclude_lists=None):
    """The runners' --mode recommend: the k next items after every user's whole known sequence (``user_seqs[u]``, the evaluation input of the
    test split, whose last item is the held-out one), excluding ``user_history[u]`` plus that last item -- everything the user is known to have
    seen.  Users are sharded over the data-parallel ranks as eval_model shards them; rank 0 writes ``path``: one line per user, in uid order,
    ``user_name \\t item_1 ... item_k \\t score_1 ... score_k`` with the item file's names (pad slots of a short list omitted).
    ``candidates``, ``candidate_lists``: as recommend's; under ``candidate_lists`` a user without a list gets no line.
    ``diversify``: as recommend's.  The file's format is unchanged; a line's scores are the items' relevance scores in the order the items were
    picked, no longer necessarily descending.  ``Log_file`` then gets one line, ``recommend_ild``: the mean intra-list diversity (mean 1 - cosine
    over a list's pairs of items) of the plain top-k lists and of the re-ranked ones, over the users with at least two items (``k of n users``).
    ``score_dtype``: as recommend's.  ``exclude_lists``: as recommend's -- added to the exclusion above, of any length."""
    n_users = len(user_seqs)
    world, rank_id, uids = _shard_users(n_users, batch_size)
    exclude = {}
    for u in uids:
        u = int(u)
        if u not in exclude:
            exclude[u] = np.concatenate([np.asarray(user_history[u], dtype=np.int64).reshape(-1), np.asarray(user_seqs[u][-1:], dtype=np.int64)])
    ids, scores, ild = _recommend(model, user_seqs, item_embeddings, k, args, exclude, uids, candidates, candidate_lists, diversify, True, score_dtype,
                                  exclude_lists)
    ids, scores = _gather_cat(ids, world), _gather_cat(scores, world)
    if ild is not None:                                            # gathered over the ranks the way the ids are
        ild = _gather_cat(ild, world)
    if rank_id != 0:
        return None
    ids, scores = ids[:n_users].cpu().numpy(), scores[:n_users].cpu().numpy()
    if ild is not None and Log_file is not None:
        pairs = (ids != 0).sum(1) >= 2                             # a list of fewer than two items has no diversity to speak of
        d = ild[:n_users].cpu().numpy().astype(np.float64)[pairs]
        plain, mmr = (float(d[:, 0].mean()), float(d[:, 1].mean())) if d.shape[0] else (0.0, 0.0)
        Log_file.info('recommend_ild   top-{} {:0.5f}   mmr(lambda {:g}, pool {}) {:0.5f}   {} of {} users'.format(
            k, plain, diversify.lam, diversify.pool, mmr, int(pairs.sum()), n_users))
    listed = np.ones(n_users, bool) if candidate_lists is None else has_candidate_list(candidate_lists, range(n_users))
    with open(path, 'w') as f:
        for u in range(n_users):
            if not listed[u]:
                continue
            keep = ids[u] != 0
            f.write(user_names[u] + '\t' + ' '.join(item_names[int(i)] for i in ids[u][keep]) + '\t'
                    + ' '.join('%.9g' % float(s) for s in scores[u][keep]) + '\n')
    return path


def read_similar_items(path, item_names):
    """A --similar_items file -> int64 array of item ids, in file order: one item name per line (``item_names`` as read_candidates').  Blank lines
    and repeats are ignored (a repeated name keeps its first place); names that are no item raise ValueError listing the first few, as
    read_candidates does; a file without any name raises as well."""
    index = {name: i for i, name in enumerate(item_names) if i > 0 and name is not None}
    ids, seen, unknown = [], set(), []
    with open(path) as f:
        for line in f:
            name = line.strip()
            if not name:
                continue
            i = index.get(name)
            if i is None:
                if name not in unknown:
                    unknown.append(name)
            elif i not in seen:
                seen.add(i)
                ids.append(i)
    if unknown:
        raise ValueError(f'{path}: {len(unknown)} name(s) that are no item of this dataset: ' + ', '.join(unknown[:5]) + (' ...' if len(unknown) > 5 else ''))
    if not ids:
        raise ValueError(f'{path}: no item name in the file')
    return np.asarray(ids, dtype=np.int64)


SIMILAR_METRICS = ('cos', 'dot')


def similar_items(item_embeddings, k, item_ids=None, candidates=None, metric='cos', min_sim=None):
    """The k nearest other items of the table for each query item.

    ``item_embeddings``: the fp32 [N + 1, E] table of ``get_item_embeddings`` / ``get_itemLMDB_embeddings`` / ``get_itemId_embeddings`` (row 0 =
    the pad item).  ``item_ids`` (default: 1 .. N): the query items, in the order of the returned rows; an id outside 1 .. N gets pad slots only,
    a repeated id an equal row.  ``metric``: 'cos' (the cosine; an all-zero or non-finite row is no one's neighbour and has none) or 'dot' (the
    scores --mode recommend ranks by).  ``candidates`` (candidate_mask's input): neighbours come from the candidate items only; a query need not
    be one.  ``min_sim``: items scoring below it are not listed (0.95 under 'cos': near-duplicates only).
    Returns (ids LongTensor [Q, k], scores fp32 [Q, k]) on the table's device: score descending, ties by smaller id, the query itself never
    listed; fewer than k neighbours: id 0 / score -inf in the remaining slots.  The rule: include/a4r_similar.h.  One a4r_topk_similar launch pair
    per batch of A4R_EVAL_USER_BATCH (default 8192) queries, the inverse norms computed once per call (a4r_row_inv_norms); neither a normalised
    copy of the table nor the [queries, items] score matrix is formed."""
    if metric not in SIMILAR_METRICS:
        raise ValueError(f'similar_items: metric {metric!r}, expected one of {SIMILAR_METRICS}')
    if min_sim is not None and math.isnan(float(min_sim)):
        raise ValueError('similar_items: min_sim is NaN')
    k = int(k)
    emb = item_embeddings.float().contiguous()
    dev = emb.device
    n1 = emb.shape[0]
    cand = candidate_mask(candidates, n1, dev)
    q = np.arange(1, n1, dtype=np.int64) if item_ids is None else np.asarray(torch.as_tensor(item_ids).cpu(), dtype=np.int64).reshape(-1)
    if q.size == 0:
        return torch.zeros(0, k, dtype=torch.long, device=dev), torch.zeros(0, k, dtype=torch.float32, device=dev)
    q32 = torch.from_numpy(np.where((q < 0) | (q > np.iinfo(np.int32).max), 0, q).astype(np.int32)).to(dev)      # (an id outside int32 names no row: a pad list)
    inv = L.row_inv_norms(emb) if metric == 'cos' else None
    step = int(os.environ.get('A4R_EVAL_USER_BATCH', 0)) or 8192          # (eval_ranks' user batch)
    out_ids, out_scores = [], []
    for a in range(0, q.size, step):
        b = min(a + step, q.size)
        ids = torch.empty(b - a, k, dtype=torch.int32, device=dev)
        scores = torch.empty(b - a, k, dtype=torch.float32, device=dev)
        L.topk_similar(emb, inv, q32[a:b], cand, min_sim, k, ids, scores)
        out_ids.append(ids.long())
        out_scores.append(scores)
    return torch.cat(out_ids), torch.cat(out_scores)


def write_similar_items(item_embeddings, k, batch_size, item_names, path, item_ids=None, candidates=None, metric='cos', min_sim=None, Log_file=None):
    """The runners' --mode similar: similar_items for the query items ``item_ids`` (default: every item 1 .. N), sharded over the data-parallel
    ranks as write_recommendations shards its users.  Rank 0 writes ``path``: one line per query item, in query order,
    ``item_name \\t name_1 ... name_k \\t score_1 ... score_k`` with the item file's names (pad slots omitted, scores as %.9g); an item without
    any neighbour gets no line.  ``Log_file`` gets one line, ``similar``: the number of query items, how many have a neighbour, and their mean
    best score.  Returns the path on rank 0, None elsewhere."""
    n1 = item_embeddings.shape[0]
    q = np.arange(1, n1, dtype=np.int64) if item_ids is None else np.asarray(item_ids, dtype=np.int64).reshape(-1)
    nq = int(q.size)
    if nq == 0:
        raise ValueError('write_similar_items: no query item')
    world, rank_id, rows = _shard_users(nq, batch_size)
    ids, scores = similar_items(item_embeddings, k, q[np.asarray(rows, dtype=np.int64)], candidates, metric, min_sim)
    ids, scores = _gather_cat(ids, world), _gather_cat(scores, world)
    if rank_id != 0:
        return None
    ids, scores = ids[:nq].cpu().numpy(), scores[:nq].cpu().numpy()
    has = ids[:, 0] != 0
    with open(path, 'w') as f:
        for r in range(nq):
            if not has[r]:
                continue
            keep = ids[r] != 0
            f.write(item_names[int(q[r])] + '\t' + ' '.join(item_names[int(i)] for i in ids[r][keep]) + '\t'
                    + ' '.join('%.9g' % float(s) for s in scores[r][keep]) + '\n')
    if Log_file is not None:
        best = float(scores[has, 0].astype(np.float64).mean()) if has.any() else 0.0
        Log_file.info('similar   top-{} lists of {} items, {} with a neighbour, mean best score {:0.5f} -> {}'.format(k, nq, int(has.sum()), best, path))
    return path


def user_vectors(model, user_seqs, item_embeddings, args, user_ids=None):
    """The user tower's vector of each listed user (default: every user of ``user_seqs``) -> fp32 [n, E] on the model's device: the last
    ``max_seq_len`` items of ``user_seqs[u]`` through ``user_encoder``, last position, in batches of A4R_EVAL_USER_BATCH (default 8192) -- the
    vectors recommend() scores the item table with (the same inputs, built by the same code)."""
    inner = _inner(model, args)
    dev = next(model.parameters()).device
    emb = item_embeddings.to(dev).float().contiguous()
    uids = np.arange(len(user_seqs), dtype=np.int64) if user_ids is None else np.asarray(user_ids, dtype=np.int64).reshape(-1)
    if uids.size == 0:
        return torch.zeros(0, emb.shape[1], dtype=torch.float32, device=dev)
    ids_np, mask_np = _user_inputs(user_seqs, uids, int(args.max_seq_len))
    step = int(os.environ.get('A4R_EVAL_USER_BATCH', 0)) or 8192          # (eval_ranks' user batch)
    out = []
    model.eval()
    with torch.no_grad():
        for a in range(0, uids.size, step):
            out.append(_encode_users(inner, emb, ids_np, mask_np, a, min(a + step, uids.size)).float())
    return torch.cat(out)


def read_audience_users(path, user_names):
    """An --audience_users file -> bool array [n_users]: one user name per line, the names --mode recommend writes (``user_names[u]``:
    preprocess.read_behavior_names).  Blank lines and repeats are ignored; names that are no user raise ValueError listing the first few, as
    read_candidates does; a file without any name raises as well."""
    index = {name: u for u, name in enumerate(user_names) if name is not None}
    mask = np.zeros(len(user_names), dtype=bool)
    unknown = []
    with open(path) as f:
        for line in f:
            name = line.strip()
            if not name:
                continue
            u = index.get(name)
            if u is None:
                if name not in unknown:
                    unknown.append(name)
            else:
                mask[u] = True
    if unknown:
        raise ValueError(f'{path}: {len(unknown)} name(s) that are no user of this dataset: ' + ', '.join(unknown[:5]) + (' ...' if len(unknown) > 5 else ''))
    if not mask.any():
        raise ValueError(f'{path}: no user name in the file')
    return mask


def audience_seen_csr(seen, n_users):
    """The users' seen lists as a4r_topk_users reads them: ``seen[u]`` (any iterable of item ids, u = 0 .. n_users - 1) -> (ptr int64
    [n_users + 2], flat int32): row 0 -- the pad row of the user table -- is empty, row u + 1 holds user u's ids ascending, each once.  There is
    no cap on a list's length.  An id below 0 or beyond int32 names no item and becomes -1 (harmless, like any id outside 1 .. N)."""
    rows = [np.zeros(0, np.int64)]
    for u in range(n_users):
        x = np.asarray(seen[u], dtype=np.int64).reshape(-1)
        rows.append(np.unique(np.where((x < 0) | (x > np.iinfo(np.int32).max), -1, x)))
    lens = np.fromiter((x.size for x in rows), dtype=np.int64, count=len(rows))
    ptr = np.zeros(len(rows) + 1, dtype=np.int64)
    np.cumsum(lens, out=ptr[1:])
    return ptr, np.concatenate(rows).astype(np.int32)


def _eligible_rows(eligible, n_users, dev):
    """``eligible`` (bool [n_users], tensor or array, or None) -> (uint8 [n_users + 1] on ``dev`` with the pad row 0 not eligible, or None; the
    number of eligible users)."""
    if eligible is None:
        return None, n_users
    m = np.asarray(eligible.cpu() if isinstance(eligible, torch.Tensor) else eligible)
    if m.ndim != 1 or m.shape[0] != n_users:
        raise ValueError(f'eligible: one entry per user expected, [{n_users}], got {tuple(m.shape)}')
    m = m != 0
    return torch.from_numpy(np.concatenate([np.zeros(1, bool), m]).astype(np.uint8)).to(dev), int(m.sum())


def _audience(table, emb, k, q, ptr, flat, elig):
    """audience's launches on a user table that stands (fp32 [n_users + 1, E], row 0 zero): the query items ``q`` (int64 array) in batches of
    A4R_EVAL_USER_BATCH, one a4r_topk_users launch pair each -> (user ids LongTensor [Q, k] = row - 1, a pad -1; scores fp32 [Q, k])."""
    dev = table.device
    if q.size == 0:
        return torch.zeros(0, k, dtype=torch.long, device=dev), torch.zeros(0, k, dtype=torch.float32, device=dev)
    q32 = torch.from_numpy(np.where((q < 0) | (q > np.iinfo(np.int32).max), 0, q).astype(np.int32)).to(dev)      # (an id outside int32 names no row: a pad list)
    step = int(os.environ.get('A4R_EVAL_USER_BATCH', 0)) or 8192          # (eval_ranks' user batch)
    out_rows, out_scores = [], []
    for a in range(0, q.size, step):
        b = min(a + step, q.size)
        rows = torch.empty(b - a, k, dtype=torch.int32, device=dev)
        scores = torch.empty(b - a, k, dtype=torch.float32, device=dev)
        L.topk_users(emb, q32[a:b], table, ptr, flat, elig, k, rows, scores)
        out_rows.append(rows.long() - 1)
        out_scores.append(scores)
    return torch.cat(out_rows), torch.cat(out_scores)


def _user_table(vectors):
    """user vectors [n, E] -> the table a4r_topk_users sweeps: [n + 1, E] with a zero pad row 0, user u in row u + 1"""
    return torch.cat([torch.zeros(1, vectors.shape[1], dtype=torch.float32, device=vectors.device), vectors.float()]).contiguous()


def audience(model, user_seqs, item_embeddings, k, args, item_ids=None, seen=None, eligible=None):
    """The k best users for each query item: whom to show the item to -- a new or cold item (the item tower gives it a vector from its content
    alone), a campaign, the seed users of an item nobody has interacted with.

    ``user_seqs[u]``: the users' item ids, as recommend's; every user is encoded (user_vectors) into one table per call.  ``item_ids`` (default:
    1 .. N): the query items, in the order of the returned rows; an id outside 1 .. N gets pad slots only, a repeated id an equal row.
    ``seen[u]`` (default: ``user_seqs[u]``): the items user u has seen -- a user is never listed for an item in it; of any length (sorted and
    de-duplicated here, audience_seen_csr: the 264-id cap of recommend's exclusion lists does not apply).  ``eligible`` (bool [n_users], or
    None): only these users are listed.
    Returns (user ids LongTensor [Q, k], scores fp32 [Q, k]) on the model's device: score descending, ties by smaller user id; fewer than k
    users: id -1 / score -inf in the remaining slots.  score(item, user) has the bits recommend() gives the same pair.  The rule:
    include/a4r_audience.h.  One a4r_topk_users launch pair per batch of A4R_EVAL_USER_BATCH (default 8192) query items; the [items, users]
    score matrix is never formed."""
    k = int(k)
    dev = next(model.parameters()).device
    emb = item_embeddings.to(dev).float().contiguous()
    n_users = len(user_seqs)
    q = np.arange(1, emb.shape[0], dtype=np.int64) if item_ids is None else np.asarray(torch.as_tensor(item_ids).cpu(), dtype=np.int64).reshape(-1)
    elig, _ = _eligible_rows(eligible, n_users, dev)
    ptr, flat = audience_seen_csr(user_seqs if seen is None else seen, n_users)
    table = _user_table(user_vectors(model, user_seqs, emb, args))
    return _audience(table, emb, k, q, torch.from_numpy(ptr).to(dev), torch.from_numpy(flat).to(dev), elig)


def write_audience(model, user_seqs, user_history, item_embeddings, k, batch_size, args, user_names, item_names, path, item_ids=None, eligible=None,
                   Log_file=None, exclude_lists=None):
    """The runners' --mode audience: the k best users of the query items ``item_ids`` (default: every item 1 .. N) among ``eligible`` (bool
    [n_users], default: every user), a user never listed for an item of ``user_history[u]`` or the last item of ``user_seqs[u]`` -- everything
    the user is known to have seen: write_recommendations' exclusion, without its 264-id cap.  The users are sharded over the data-parallel
    ranks for the user tower and their vectors gathered as get_item_embeddings gathers its shards; the query items are sharded as
    write_similar_items shards them.  ``exclude_lists`` ({uid: item ids}, of any length): merged into the seen lists.  Rank 0 writes ``path``: one line per query item that has at least one user, in query order,
    ``item_name \\t user_1 ... user_k \\t score_1 ... score_k`` (pad slots omitted, scores as %.9g).  ``Log_file`` gets one line, ``audience``.
    Returns the path on rank 0, None elsewhere."""
    k = int(k)
    dev = next(model.parameters()).device
    emb = item_embeddings.to(dev).float().contiguous()
    n_users = len(user_seqs)
    q = np.arange(1, emb.shape[0], dtype=np.int64) if item_ids is None else np.asarray(item_ids, dtype=np.int64).reshape(-1)
    nq = int(q.size)
    if nq == 0:
        raise ValueError('write_audience: no query item')
    if n_users == 0:
        raise ValueError('write_audience: no user')
    elig, n_elig = _eligible_rows(eligible, n_users, dev)
    lo, hi, chunk, world = _my_shard(n_users)
    table = _user_table(_gather_shards(user_vectors(model, user_seqs, emb, args, np.arange(lo, hi, dtype=np.int64)), n_users, chunk, world))
    seen = [np.concatenate([np.asarray(user_history[u], dtype=np.int64).reshape(-1), np.asarray(user_seqs[u][-1:], dtype=np.int64)]) for u in range(n_users)]
    if exclude_lists is not None:
        seen = [np.concatenate([x, _id_array(exclude_lists[u])]) if exclude_lists.get(u) is not None else x for u, x in enumerate(seen)]
    ptr, flat = audience_seen_csr(seen, n_users)
    world, rank_id, rows = _shard_users(nq, batch_size)
    ids, scores = _audience(table, emb, k, q[np.asarray(rows, dtype=np.int64)], torch.from_numpy(ptr).to(dev), torch.from_numpy(flat).to(dev), elig)
    ids, scores = _gather_cat(ids, world), _gather_cat(scores, world)
    if rank_id != 0:
        return None
    ids, scores = ids[:nq].cpu().numpy(), scores[:nq].cpu().numpy()
    has = ids[:, 0] >= 0
    with open(path, 'w') as f:
        for r in range(nq):
            if not has[r]:
                continue
            keep = ids[r] >= 0
            f.write(item_names[int(q[r])] + '\t' + ' '.join(user_names[int(u)] for u in ids[r][keep]) + '\t'
                    + ' '.join('%.9g' % float(s) for s in scores[r][keep]) + '\n')
    if Log_file is not None:
        best = float(scores[has, 0].astype(np.float64).mean()) if has.any() else 0.0
        Log_file.info('audience   top-{} lists of {} items over {} users ({} eligible), {} with a user, mean best score {:0.5f} -> {}'.format(
            k, nq, n_users, n_elig, int(has.sum()), best, path))
    return path
