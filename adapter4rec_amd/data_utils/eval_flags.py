"""The flags that restrict or re-rank what evaluation and recommendation range over (--topk .. --eval_negatives_out) and those of --mode similar
(--similar_*) and --mode audience (--audience_*) and the exclusion lists of --mode recommend / audience (--exclude_*), for both entry points (run.py, cv/run_adapter.py): their declaration, their refusals, and their
translation into the arguments of data_utils.metrics (eval_model's restriction, write_recommendations', write_similar_items' and write_audience's
calls).  No kernel is called from here."""
import math
import os

import torch.distributed as dist

from .._lib_diversify import MMR_MAX_POOL
from .._lib_user_lists import LIST_MAX
from .metrics import (SCORE_DTYPES, SIMILAR_METRICS, Diversify, EvalNegatives, candidate_mask, item_counts, merge_exclude_lists, read_candidate_lists,
                      read_candidates, read_audience_users, read_exclude_lists, read_full_histories, read_similar_items, write_audience,
                      write_eval_negatives, write_recommendations, write_similar_items)
from .preprocess import read_behavior_names

EXCLUDE_HISTORIES = ('window', 'full')       # --exclude_history: the reader's window of a user's line (the exclusion as it was), or the whole line


def add_eval_flags(p):
    p.add_argument('--topk', type=int, default=10)                     # --mode recommend: items per user
    p.add_argument('--recommend_out', type=str, default=None)          # --mode recommend: output file (default <model_dir>/recommend_<load_ckpt_name>.tsv)
    p.add_argument('--candidate_items', type=str, default=None)        # --mode test / recommend: a file of item names, one per line -- rank and recommend among these items only
    p.add_argument('--candidate_lists', type=str, default=None)        # --mode test / recommend: a file of `user_name \t item_name item_name ...` lines -- rank and recommend within each user's own list
    p.add_argument('--diversify', type=str, default='none', choices=['none', 'mmr'])      # --mode recommend: mmr = re-rank each user's --mmr_pool best items by maximal marginal relevance, near-duplicates give way
    p.add_argument('--mmr_lambda', type=float, default=0.7)            # the weight of relevance against similarity to the items already picked, in [0, 1]; 1 = the plain list
    p.add_argument('--mmr_pool', type=int, default=100)                # how many of the best items the --topk picks are made from: --topk .. 256
    p.add_argument('--eval_negatives', type=int, default=0)            # --mode test / the per-epoch evaluation: rank each target among N negatives drawn on the device (0 = off: the whole catalogue; at most 4096)
    p.add_argument('--eval_neg_sampling', type=str, default='uniform', choices=['uniform', 'pop'])      # pop: in proportion to an item's occurrences in the training sequences
    p.add_argument('--eval_neg_seed', type=int, default=20240607)      # the seed of the draws: the same negatives in every epoch, batch size and world size
    p.add_argument('--eval_negatives_out', type=str, default=None)     # --mode test: write the test split's drawn negatives as a --candidate_lists file
    p.add_argument('--similar_out', type=str, default=None)            # --mode similar: output file (default <model_dir>/similar_<load_ckpt_name>.tsv)
    p.add_argument('--similar_items', type=str, default=None)          # --mode similar: a file of item names, one per line -- the query items, in file order (default: every item)
    p.add_argument('--similar_metric', type=str, default='cos', choices=list(SIMILAR_METRICS))      # --mode similar: cosine, or the dot product --mode recommend ranks by
    p.add_argument('--similar_min', type=float, default=None)          # --mode similar: list only the items scoring at least this (0.95 under cos: near-duplicates)
    p.add_argument('--audience_out', type=str, default=None)           # --mode audience: output file (default <model_dir>/audience_<load_ckpt_name>.tsv)
    p.add_argument('--audience_items', type=str, default=None)         # --mode audience: a file of item names, one per line -- the query items, in file order (default: every item)
    p.add_argument('--audience_users', type=str, default=None)         # --mode audience: a file of user names, one per line -- the eligible users (default: every user)
    p.add_argument('--score_dtype', type=str, default='fp32', choices=list(SCORE_DTYPES))      # --mode test / recommend and the per-epoch evaluation: bf16 = score against the item table on the bf16 MFMA (operands rounded, fp32 sums)
    p.add_argument('--exclude_lists', type=str, default=None)          # --mode recommend / audience: a file of `user_name \t item_name item_name ...` lines -- items never recommended to the user, of any number
    p.add_argument('--exclude_history', type=str, default='window', choices=list(EXCLUDE_HISTORIES))      # --mode recommend / audience: full = exclude every item of the user's whole line of the behaviours file, not only the last max_seq_len + 3


def check_flags(args):
    """Both entry points' refusals, before anything is set up (no device, no process group)."""
    check_candidate_flag(args)
    check_eval_negatives_flag(args)
    check_diversify_flag(args)
    check_similar_flag(args)
    check_audience_flag(args)
    check_score_dtype_flag(args)
    check_exclude_flag(args)                 # (last: every message above keeps its precedence)


def check_exclude_flag(args):
    """--exclude_lists FILE and --exclude_history full are honoured by --mode recommend and --mode audience, alone, together (their union is
    excluded) and beside --candidate_items and --diversify mmr; under any other mode, beside --candidate_lists (a shortlist is filtered where it
    is made) and beside --score_dtype bf16 (a4r_topk_items_excl scores in fp32 only) they are refused instead of ignored."""
    given = []
    if getattr(args, 'exclude_lists', None):
        given.append('--exclude_lists')
    if getattr(args, 'exclude_history', 'window') != 'window':
        given.append(f'--exclude_history {args.exclude_history}')
    for flag in given:
        if args.mode not in ('recommend', 'audience'):
            raise ValueError(f'{flag} is honoured by --mode recommend and --mode audience only, not by --mode {args.mode}')
        if getattr(args, 'candidate_lists', None):
            raise ValueError(f'{flag} and --candidate_lists cannot be combined: a shortlist is filtered where it is made')
        if getattr(args, 'score_dtype', 'fp32') != 'fp32':
            raise ValueError(f'{flag} and --score_dtype {args.score_dtype} cannot be combined: a4r_topk_items_excl scores in fp32 only')


def exclude_lists_from_args(args, behaviors_path, name2id, user_names, item_names, Log_file):
    """--exclude_lists FILE / --exclude_history full -> the ``exclude_lists`` keyword of write_recommendations / write_audience: {} without
    either flag (the calls are then the ones made before), else the union of the file's lists and the users' whole lines of the behaviours
    file, and one log line."""
    lists, sources, bad_users, bad_items = None, [], 0, 0
    if getattr(args, 'exclude_history', 'window') == 'full':
        lists, bu, bi = read_full_histories(behaviors_path, name2id, user_names, item_names)
        sources.append(f'{behaviors_path} (--exclude_history full)')
        bad_users, bad_items = bad_users + bu, bad_items + bi
    if getattr(args, 'exclude_lists', None):
        more, bu, bi = read_exclude_lists(args.exclude_lists, user_names, item_names)
        lists = merge_exclude_lists(lists, more)
        sources.append(args.exclude_lists)
        bad_users, bad_items = bad_users + bu, bad_items + bi
    if lists is None:
        return {}
    lens = [len(set(v)) for v in lists.values()]
    Log_file.info(f'exclude lists: {len(lists)} users, {sum(lens)} ids in all, longest {max(lens, default=0)}; {bad_users} user names and {bad_items} item names '
                  f'unknown, skipped <- {" + ".join(sources)}')
    return dict(exclude_lists=lists)


def check_score_dtype_flag(args):
    """--score_dtype bf16 is honoured by --mode test, the per-epoch evaluation of --mode train and --mode recommend, alone or beside
    --candidate_items; beside --candidate_lists, --eval_negatives, --diversify mmr and under --mode similar it is refused instead of ignored:
    their kernels score in fp32 only.  --ce_dtype is independent of it."""
    if getattr(args, 'score_dtype', 'fp32') == 'fp32':
        return
    if args.mode == 'similar':
        raise ValueError('--score_dtype bf16 is not honoured by --mode similar: a4r_topk_similar scores in fp32 only')
    if args.mode == 'audience':
        raise ValueError('--score_dtype bf16 is not honoured by --mode audience: a4r_topk_users scores in fp32 only')
    if getattr(args, 'candidate_lists', None):
        raise ValueError('--score_dtype bf16 and --candidate_lists cannot be combined: the kernels of a user\'s own list score in fp32 only')
    if int(getattr(args, 'eval_negatives', 0) or 0) != 0:
        raise ValueError('--score_dtype bf16 and --eval_negatives cannot be combined: the sampled evaluation scores in fp32 only')
    if getattr(args, 'diversify', 'none') != 'none':
        raise ValueError(f'--score_dtype bf16 and --diversify {args.diversify} cannot be combined: the re-ranking scores in fp32 only')


def score_dtype_from_args(args, Log_file):
    """--score_dtype as the ``score_dtype`` keyword of eval_model / write_recommendations: {} under the default (the calls are then the ones made
    before), else the keyword, and one log line naming the dtype."""
    if getattr(args, 'score_dtype', 'fp32') == 'fp32':
        return {}
    Log_file.info(f'score dtype: {args.score_dtype} (item-table scores on the bf16 MFMA: operands rounded to nearest even, fp32 sums)')
    return dict(score_dtype=args.score_dtype)


def check_similar_flag(args):
    """--mode similar lists items, not users: the flags of per-user restriction, re-ranking and evaluation are refused under it instead of
    ignored (--candidate_items is honoured: neighbours come from the set), and --similar_out / --similar_items / --similar_metric /
    --similar_min are refused under every other mode."""
    if args.mode != 'similar':
        for flag, default in (('similar_out', None), ('similar_items', None), ('similar_metric', 'cos'), ('similar_min', None)):
            if getattr(args, flag, default) != default:
                raise ValueError(f'--{flag} is honoured by --mode similar only, not by --mode {args.mode}')
        return
    if getattr(args, 'candidate_lists', None):
        raise ValueError('--candidate_lists is a list per user: it is not honoured by --mode similar (--candidate_items is)')
    if getattr(args, 'diversify', 'none') != 'none':
        raise ValueError(f'--diversify {args.diversify} re-ranks the lists of users: it is not honoured by --mode similar')
    if int(getattr(args, 'eval_negatives', 0) or 0) != 0:
        raise ValueError('--eval_negatives is an evaluation protocol: it is not honoured by --mode similar')
    if args.similar_min is not None and math.isnan(float(args.similar_min)):
        raise ValueError('--similar_min nan: not a number')


def check_audience_flag(args):
    """--mode audience lists users for items: the flags that restrict, re-rank or evaluate the lists of users' items and those of --mode similar
    are refused under it instead of ignored (--candidate_items / --candidate_lists: check_candidate_flag; --score_dtype bf16:
    check_score_dtype_flag), and --audience_out / --audience_items /
    --audience_users are refused under every other mode."""
    if args.mode != 'audience':
        for flag in ('audience_out', 'audience_items', 'audience_users'):
            if getattr(args, flag, None) is not None:
                raise ValueError(f'--{flag} is honoured by --mode audience only, not by --mode {args.mode}')
        return
    if getattr(args, 'diversify', 'none') != 'none':
        raise ValueError(f'--diversify {args.diversify} re-ranks the lists of users: it is not honoured by --mode audience')
    if int(getattr(args, 'eval_negatives', 0) or 0) != 0 or getattr(args, 'eval_negatives_out', None):
        raise ValueError('--eval_negatives is an evaluation protocol: it is not honoured by --mode audience')
    for flag, default in (('eval_neg_sampling', 'uniform'), ('eval_neg_seed', 20240607)):
        if getattr(args, flag, default) != default:
            raise ValueError(f'--{flag} belongs to --eval_negatives, an evaluation protocol: it is not honoured by --mode audience')


def check_candidate_flag(args):
    """--candidate_items and --candidate_lists restrict --mode test and --mode recommend; training and its per-epoch evaluation are not
    restricted by them, so any other mode refuses either flag instead of ignoring it.  The two together are refused as well: a user's own list
    is the restriction, not one more beside a shared set."""
    for flag in ('candidate_items', 'candidate_lists'):
        if getattr(args, flag, None) and not ('test' in args.mode or args.mode in ('recommend', 'similar')):
            raise ValueError(f'--{flag} is honoured by --mode test and --mode recommend only, not by --mode {args.mode} '
                             '(training and its per-epoch evaluation range over the whole catalogue)')
    if getattr(args, 'candidate_items', None) and getattr(args, 'candidate_lists', None):
        raise ValueError('--candidate_lists (a list per user) and --candidate_items (one set for all users) cannot be combined: give one of them')


def check_eval_negatives_flag(args):
    """--eval_negatives N (with --eval_neg_sampling / --eval_neg_seed) is honoured by --mode test and by the per-epoch evaluation of training;
    it is refused under --mode recommend and beside --candidate_items / --candidate_lists (a user's drawn negatives are the restriction), and
    --eval_negatives_out is --mode test's."""
    n = int(getattr(args, 'eval_negatives', 0) or 0)
    out = getattr(args, 'eval_negatives_out', None)
    if n == 0:
        if out:
            raise ValueError('--eval_negatives_out needs --eval_negatives N')
        return
    if not 1 <= n <= LIST_MAX:
        raise ValueError(f'--eval_negatives {n}: outside 1 .. {LIST_MAX}')
    if args.mode == 'recommend':
        raise ValueError('--eval_negatives is an evaluation protocol: it is not honoured by --mode recommend')
    for flag in ('candidate_items', 'candidate_lists'):
        if getattr(args, flag, None):
            raise ValueError(f'--eval_negatives and --{flag} cannot be combined: the drawn negatives are the candidates '
                             '(to replay a draw, write it with --eval_negatives_out and give the file to --candidate_lists alone)')
    if out and 'test' not in args.mode:
        raise ValueError(f'--eval_negatives_out is honoured by --mode test only, not by --mode {args.mode}')
    if not 0 <= int(args.eval_neg_seed) < 2 ** 64:
        raise ValueError(f'--eval_neg_seed {args.eval_neg_seed}: outside 0 .. 2^64 - 1')


def check_diversify_flag(args):
    """--diversify mmr (with --mmr_lambda / --mmr_pool) re-ranks the lists of --mode recommend; every other mode refuses it instead of ignoring
    it.  The pool is a top-K output that the --topk list is cut from: topk <= pool <= 256."""
    if getattr(args, 'diversify', 'none') == 'none':
        return
    if args.mode != 'recommend':
        raise ValueError(f'--diversify {args.diversify} is honoured by --mode recommend only, not by --mode {args.mode}')
    lam = float(args.mmr_lambda)
    if math.isnan(lam) or not 0.0 <= lam <= 1.0:
        raise ValueError(f'--mmr_lambda {args.mmr_lambda}: outside [0, 1]')
    if not int(args.topk) <= int(args.mmr_pool) <= MMR_MAX_POOL:
        raise ValueError(f'--mmr_pool {args.mmr_pool}: outside --topk = {args.topk} .. {MMR_MAX_POOL}')


def _candidates_from_args(args, user_names, item_names, Log_file):
    """--candidate_items FILE / --candidate_lists FILE -> (bool array [item_num + 1] or None, {uid: [item ids]} or None) in the numbering
    read_behaviors gives users and items (``user_names``, ``item_names``: preprocess.read_behavior_names)."""
    mask = lists = None
    if getattr(args, 'candidate_items', None):
        mask = read_candidates(args.candidate_items, item_names)
        Log_file.info(f'candidate items: {int(mask.sum())} of {len(item_names) - 1} from {args.candidate_items}')
    if getattr(args, 'candidate_lists', None):
        lists = read_candidate_lists(args.candidate_lists, user_names, item_names)
        Log_file.info(f'candidate lists: {len(lists)} of {len(user_names)} users, {sum(len(v) for v in lists.values())} items in all, from {args.candidate_lists}')
    return mask, lists


def eval_negatives_from_args(args, users_train, item_num, Log_file):
    """--eval_negatives N -> an EvalNegatives, or None without the flag (then nothing changes)."""
    n = int(getattr(args, 'eval_negatives', 0) or 0)
    if n == 0:
        return None
    pop = args.eval_neg_sampling == 'pop'
    spec = EvalNegatives(n, seed=args.eval_neg_seed, counts=item_counts(users_train, item_num) if pop else None)
    Log_file.info(f'eval negatives: {n} per user, {args.eval_neg_sampling} sampling, seed {spec.seed}'
                  + (f', {int((spec.counts > 0).sum())} of {item_num} items with a training occurrence' if pop else ''))
    return spec


def eval_restriction(args, behaviors_path, name2id, users_train, hist_test, users_test, item_num, dev, Log_file):
    """The flags as eval_model's restriction keywords, for every evaluation of a run: {} without a flag (the calls are then the ones made
    before), else one of ``candidates`` (--candidate_items: the mask uploaded to ``dev`` here, once for both splits), ``candidate_lists``
    (--candidate_lists) and ``eval_negatives`` (--eval_negatives; with --eval_negatives_out, rank 0 writes the test split's draws), and beside
    none or ``candidates``, ``score_dtype`` (--score_dtype bf16).  check_flags
    has refused every pair of them, and the candidate flags outside --mode test.  The behaviours file is read for its names at most once."""
    out = getattr(args, 'eval_negatives_out', None) and dist.get_rank() == 0
    user_names = item_names = None
    if getattr(args, 'candidate_items', None) or getattr(args, 'candidate_lists', None) or out:
        user_names, item_names = read_behavior_names(behaviors_path, name2id, args.max_seq_len, args.min_seq_len)
    mask, lists = _candidates_from_args(args, user_names, item_names, Log_file)
    kw = {} if mask is None else dict(candidates=candidate_mask(mask, item_num + 1, dev))
    if lists is not None:
        kw = dict(candidate_lists=lists)
    neg = eval_negatives_from_args(args, users_train, item_num, Log_file)
    if neg is not None:
        kw = dict(eval_negatives=neg)
        if out:
            k = write_eval_negatives(neg, hist_test, users_test, item_num + 1, args, user_names, item_names, args.eval_negatives_out, dev)
            Log_file.info(f'eval negatives: the draws of the test split for {k} users -> {args.eval_negatives_out}')
    kw.update(score_dtype_from_args(args, Log_file))
    return kw


def recommend_out_path(args, model_dir):
    return args.recommend_out or os.path.join(model_dir, f'recommend_{args.load_ckpt_name}.tsv')


def write_recommend_mode(args, model, users_test, hist_test, item_embeddings, batch_size, behaviors_path, name2id, model_dir, Log_file):
    """The tail of --mode recommend in both entry points: the --topk next items after every user's whole known sequence of the test split, within
    --candidate_items / --candidate_lists and re-ranked under --diversify mmr, without the items of --exclude_lists / --exclude_history full,
    written by rank 0 to --recommend_out under the names of the behaviours file."""
    user_names, item_names = read_behavior_names(behaviors_path, name2id, args.max_seq_len, args.min_seq_len)
    mask, lists = _candidates_from_args(args, user_names, item_names, Log_file)
    spec = None
    if getattr(args, 'diversify', 'none') != 'none':
        spec = Diversify(args.mmr_lambda, args.mmr_pool)
        Log_file.info(f'diversify: mmr, lambda {spec.lam:g}, pool {spec.pool}')
    out = write_recommendations(model, users_test, hist_test, item_embeddings, args.topk, batch_size, args, user_names, item_names,
                                recommend_out_path(args, model_dir), candidates=mask, candidate_lists=lists, diversify=spec, Log_file=Log_file,
                                **score_dtype_from_args(args, Log_file),
                                **exclude_lists_from_args(args, behaviors_path, name2id, user_names, item_names, Log_file))
    if out:
        Log_file.info(f'recommend: top-{args.topk} lists of {len(users_test)} users -> {out}')


def similar_out_path(args, model_dir):
    return args.similar_out or os.path.join(model_dir, f'similar_{args.load_ckpt_name}.tsv')


def write_similar_mode(args, item_embeddings, batch_size, behaviors_path, name2id, model_dir, Log_file):
    """The tail of --mode similar in both entry points: the --topk nearest items of every item (or of --similar_items' items, in file order) by
    --similar_metric, within --candidate_items and not below --similar_min, written by rank 0 to --similar_out under the names of the item
    file.  No user is encoded."""
    _, item_names = read_behavior_names(behaviors_path, name2id, args.max_seq_len, args.min_seq_len)
    mask, _ = _candidates_from_args(args, None, item_names, Log_file)
    query = None
    if getattr(args, 'similar_items', None):
        query = read_similar_items(args.similar_items, item_names)
        Log_file.info(f'similar items: {query.size} of {len(item_names) - 1} from {args.similar_items}')
    write_similar_items(item_embeddings, args.topk, batch_size, item_names, similar_out_path(args, model_dir), item_ids=query, candidates=mask,
                        metric=args.similar_metric, min_sim=args.similar_min, Log_file=Log_file)


def audience_out_path(args, model_dir):
    return args.audience_out or os.path.join(model_dir, f'audience_{args.load_ckpt_name}.tsv')


def write_audience_mode(args, model, users_test, hist_test, item_embeddings, batch_size, behaviors_path, name2id, model_dir, Log_file):
    """The tail of --mode audience in both entry points: the --topk best users of every item (or of --audience_items' items, in file order) among
    every user (or --audience_users' users), a user never listed for an item of the user's known sequence, written by rank 0 to --audience_out
    under the names of the behaviours file."""
    user_names, item_names = read_behavior_names(behaviors_path, name2id, args.max_seq_len, args.min_seq_len)
    query = eligible = None
    if getattr(args, 'audience_items', None):
        query = read_similar_items(args.audience_items, item_names)
        Log_file.info(f'audience items: {query.size} of {len(item_names) - 1} from {args.audience_items}')
    if getattr(args, 'audience_users', None):
        eligible = read_audience_users(args.audience_users, user_names)
        Log_file.info(f'audience users: {int(eligible.sum())} of {len(user_names)} from {args.audience_users}')
    write_audience(model, users_test, hist_test, item_embeddings, args.topk, batch_size, args, user_names, item_names,
                   audience_out_path(args, model_dir), item_ids=query, eligible=eligible, Log_file=Log_file,
                   **exclude_lists_from_args(args, behaviors_path, name2id, user_names, item_names, Log_file))
