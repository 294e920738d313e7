"""fp64 numpy restatement of the full-softmax cross-entropy head of the ID tower (include/a4r.h: a4r_score_ce_*).

Rows r < R with vectors prec [R, E]; candidates are the items 1 .. N of table [N + 1, E] (row 0 is the pad row and never a candidate).
    s[r, i] = <prec[r], table[i]>,  lse_r = log sum_{i = 1 .. N} exp s[r, i]
    trained(r) = log_mask[r] != 0 and tgt[r] != 0;  count = number of trained rows;  w[r] = 1 / count on trained rows, else 0
    loss = sum_r w[r] (lse_r - s[r, tgt_r])
    d_prec[r]  = w[r] (sum_i p[r, i] table[i] - table[tgt_r]),  p = exp(s - lse_r)
    d_table[i] = sum_r w[r] (p[r, i] - [i == tgt_r]) prec[r],  i >= 1;  d_table[0] = 0
count == 0: the loss and every gradient are exactly 0."""
import numpy as np


def reference(prec, table, tgt, log_mask):
    """-> dict(loss, lse [R], s_tgt [R] (0 where tgt is 0), d_prec [R, E], d_table [N + 1, E], count, s [R, N]); all fp64."""
    prec, table = np.asarray(prec, np.float64), np.asarray(table, np.float64)
    tgt, log_mask = np.asarray(tgt, np.int64).reshape(-1), np.asarray(log_mask).reshape(-1)
    R, N1 = prec.shape[0], table.shape[0]
    assert tgt.shape == (R,) and log_mask.shape == (R,) and N1 >= 2 and np.all((tgt >= 0) & (tgt < N1))
    s = prec @ table[1:].T                                              # [R, N]: column j is item j + 1
    mx = s.max(1)
    lse = mx + np.log(np.exp(s - mx[:, None]).sum(1))
    has = tgt != 0
    rows = np.arange(R)
    s_tgt = np.where(has, s[rows, np.maximum(tgt, 1) - 1], 0.0)
    trained = (log_mask != 0) & has
    count = int(trained.sum())
    w = trained / count if count else np.zeros(R)
    loss = float(np.sum(w * (lse - s_tgt)))
    coef = np.exp(s - lse[:, None])
    coef[rows[has], tgt[has] - 1] -= 1.0
    coef *= w[:, None]
    d_table = np.zeros_like(table)
    d_table[1:] = coef.T @ prec
    return dict(loss=loss, lse=lse, s_tgt=s_tgt, d_prec=coef @ table[1:], d_table=d_table, count=count, s=s)
