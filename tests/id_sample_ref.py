"""a4r_id_sample restated on the CPU (include/a4r.h): the counter hash of oracle/dropout_masks.py, a 128-bit product in Python ints and the
skip loop over the user's sorted distinct ids.  Shared by the CPU tests (properties of the rule, the runner on the simulated library) and the GPU
tests (the kernel must give these bits)."""
import numpy as np
import torch

from oracle.dropout_masks import hash64

SAMPLE_SITE = 7001          # A4R_SAMPLE_SITE (adapter4rec_amd/csrc/a4r_common.h)


def user_negatives(seq_row, u, item_num, seed, draw):
    """seq_row: int32 [L], left-padded with 0 -> (int64 [L]: the negative of every position l < L-1 with seq_row[l] != 0, 0 elsewhere; m).
    m < 1: no candidate, all zeros."""
    row = np.asarray(seq_row, dtype=np.int32)
    L = row.shape[0]
    D = np.unique(row[row != 0])                                   # ascending, distinct (signed order, as the kernel compares)
    m = int(item_num) - len(D)
    neg = np.zeros(L, dtype=np.int64)
    if m < 1:
        return neg, m
    ls = np.flatnonzero(row[:L - 1] != 0)
    idx = [(int(draw) << 40) | (int(u) << 8) | int(l) for l in ls]
    h = hash64(seed, SAMPLE_SITE, np.array(idx, dtype=np.uint64))
    x = np.array([((int(hv) * m) >> 64) + 1 for hv in h], dtype=np.int64)         # the high half of the 64 x 64-bit product
    for s in D:
        x += x >= int(s)
    neg[ls] = x
    return neg, m


def id_sample(seqs, rows, item_num, seed, draw, negatives):
    """numpy in, numpy out: (ids int64 [B, L, 2], log_mask fp32 [B, L - 1], err)."""
    seqs = np.asarray(seqs, dtype=np.int32)
    rows = np.asarray(rows, dtype=np.int32)
    n_users, L = seqs.shape
    B = rows.shape[0]
    assert 2 <= L <= 256 and B >= 1 and n_users >= 1 and item_num >= 1 and 0 <= draw < 2 ** 24
    ids = np.zeros((B, L, 2), dtype=np.int64)
    log_mask = np.zeros((B, L - 1), dtype=np.float32)
    err = 0
    cache = {}
    for b, u in enumerate(rows.tolist()):
        if not 0 <= u < n_users:                                   # a row of pads; the table is not read
            err += 1
            continue
        ids[b, :, 0] = seqs[u]
        log_mask[b] = seqs[u, :L - 1] != 0
        if negatives:
            if u not in cache:
                cache[u] = user_negatives(seqs[u], u, item_num, seed, draw)
            neg, m = cache[u]
            err += m < 1
            ids[b, :, 1] = neg
    return ids, log_mask, int(err)


def lib_id_sample(seqs, rows, item_num, seed, draw, negatives, ids, log_mask, err):
    """The mirror behind _lib.id_sample's signature (host tensors): the stand-in of the library in the runner's CPU test."""
    i, m, e = id_sample(seqs.numpy(), rows.numpy(), item_num, seed, draw, negatives)
    assert tuple(ids.shape) == i.shape and tuple(log_mask.shape) == m.shape and ids.dtype == torch.int64 and log_mask.dtype == torch.float32
    ids.copy_(torch.from_numpy(i))
    log_mask.copy_(torch.from_numpy(m))
    err[0] = e
