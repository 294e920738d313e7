"""ctypes binding of the cross-entropy head on the bf16 MFMA (--ce_dtype bf16): the a4r_score_ce_bf16_* exports of liba4r_hip.so, declared in
include/a4r_score_ce_bf16.h (which include/a4r.h includes).  Same rules as adapter4rec_amd/_lib.py, whose names these wrappers are also reachable
under: raw device pointers, torch's current stream, no fallback.  _lib.lib() checks and installs the signature table below when it loads the
library, beside its own; tests/test_score_ce_bf16_cpu.py holds it against the header prototype by prototype."""
import ctypes as C

import torch

from . import _lib as L

SCORE_CE_BF16_E = (64, 128)   # table widths of the bf16 cross-entropy head
SCORE_CE_BF16_ROWS = 64       # A4R_SCORE_CE_BF16_ROWS: the rows a workgroup of the bf16 head holds

_P, _I, _L, _F, _SZ = C.c_void_p, C.c_int, C.c_int64, C.c_float, C.c_size_t
SCORE_CE_BF16_SIGNATURES = {
    'a4r_score_ce_bf16_cast': (_I, (_P, _P, _P, _L)),
    'a4r_score_ce_bf16_ws_bytes': (_SZ, (_I, _I, _I, _I)),
    'a4r_score_ce_bf16_ranges': (_I, (_I, _I)),
    'a4r_score_ce_bf16_fwd': (_I, (_P,) * 9 + (_I,) * 4),
    'a4r_score_ce_bf16_bwd_rows': (_I, (_P,) * 7 + (_F, _P, _P, _P) + (_I,) * 4),
    'a4r_score_ce_bf16_bwd_items': (_I, (_P,) * 7 + (_F, _P, _P) + (_I,) * 4),
}

def cast_bf16(src, dst, n=None):
    """a4r_score_ce_bf16_cast: dst (bf16, contiguous) <- the first n elements of src (fp32, contiguous) rounded to nearest even; n: all of src."""
    L.require_gpu(src, dst)
    n = src.numel() if n is None else n
    assert src.dtype == torch.float32 and dst.dtype == torch.bfloat16 and src.is_contiguous() and dst.is_contiguous()
    assert src.numel() >= n and dst.numel() >= n
    L._check(L.lib().a4r_score_ce_bf16_cast(L._stream(), L._p(src), L._p(dst), n), 'a4r_score_ce_bf16_cast')


def score_ce_bf16_ranges(R, N1):
    """score_ce_ranges for the bf16 head, whose workgroups hold SCORE_CE_BF16_ROWS rows."""
    k = int(L.lib().a4r_score_ce_bf16_ranges(R, N1))
    if k < 1:
        raise ValueError(f'score_ce_bf16_ranges: R = {R} rows and N1 = {N1} table rows (row 0 = the pad item): need R >= 1, N1 >= 2')
    return k


def score_ce_bf16_ws_bytes(R, N1, E, ranges=0):
    """Bytes of the workspace a4r_score_ce_bf16_fwd / _bwd_rows share (a host-side query); ranges 0 = the library's choice.  0 for arguments
    the kernels refuse.  Independent of N1 at a fixed range count."""
    return int(L.lib().a4r_score_ce_bf16_ws_bytes(R, N1, E, ranges))


def _score_ce_bf16_ws(prec_b, R, N1, E, ranges, ws):
    if ws is None:
        ws = torch.empty(max(score_ce_bf16_ws_bytes(R, N1, E, ranges), 16), dtype=torch.uint8, device=prec_b.device)
    assert ws.is_contiguous() and ws.numel() * ws.element_size() >= score_ce_bf16_ws_bytes(R, N1, E, ranges)
    return ws


def _score_ce_bf16_check(prec_b, table_b, tgt, log_mask, R):
    L.require_gpu(prec_b, table_b, tgt, log_mask)
    assert prec_b.dim() == 2 and table_b.dim() == 2 and prec_b.dtype == torch.bfloat16 and table_b.dtype == torch.bfloat16
    assert prec_b.is_contiguous() and table_b.is_contiguous() and prec_b.shape[1] == table_b.shape[1] and prec_b.shape[0] >= R
    assert tgt.dtype == torch.int32 and tgt.is_contiguous() and tgt.numel() >= R
    assert log_mask.dtype == torch.float32 and log_mask.is_contiguous() and log_mask.numel() >= R


def score_ce_bf16_fwd(prec_b, table_b, tgt, log_mask, lse, s_tgt, loss_ws, R, ranges=0, ws=None):
    """a4r_score_ce_bf16_fwd: score_ce_fwd on the bf16 MFMA.  prec_b [>= R, E] and table_b [N1, E] are the bf16 (RNE) copies of the fp32
    operands (cast_bf16); the outputs, the workspace (score_ce_bf16_ws_bytes) and the refusals are score_ce_fwd's (include/a4r.h)."""
    _score_ce_bf16_check(prec_b, table_b, tgt, log_mask, max(R, 0))
    L.require_gpu(lse, s_tgt, loss_ws)
    assert all(t.dtype == torch.float32 and t.is_contiguous() for t in (lse, s_tgt, loss_ws)) and lse.numel() >= R and s_tgt.numel() >= R and loss_ws.numel() >= 4
    N1, E = table_b.shape
    ws = _score_ce_bf16_ws(prec_b, R, N1, E, ranges, ws)
    L._check(L.lib().a4r_score_ce_bf16_fwd(L._stream(), L._p(prec_b), L._p(table_b), L._p(tgt), L._p(log_mask), L._p(lse), L._p(s_tgt), L._p(loss_ws), L._p(ws), R, N1, E, ranges),
           'a4r_score_ce_bf16_fwd')


def score_ce_bf16_bwd(prec_b, table_b, tgt, log_mask, lse, loss_ws, loss_scale, d_prec, d_table, R, ranges=0, scale_dev=None, ws=None):
    """The two backward launches of the bf16 cross-entropy head, shaped as score_ce_bwd: a4r_score_ce_bf16_bwd_rows overwrites d_prec (fp32 [>= R, E];
    None: skipped), a4r_score_ce_bf16_bwd_items ADDS into d_table (fp32 [N1, >= E], row 0 untouched; None: skipped).  The gradients are those
    with respect to the bf16 operands, for the fp32 masters to take as they are."""
    _score_ce_bf16_check(prec_b, table_b, tgt, log_mask, max(R, 0))
    L.require_gpu(lse, loss_ws, d_prec, d_table, scale_dev)
    assert scale_dev is None or (scale_dev.dtype == torch.float32 and scale_dev.numel() == 1)
    N1, E = table_b.shape
    if d_prec is not None:
        assert d_prec.dtype == torch.float32 and d_prec.is_contiguous() and d_prec.shape[1] == E and d_prec.shape[0] >= R
        ws = _score_ce_bf16_ws(prec_b, R, N1, E, ranges, ws)
        L._check(L.lib().a4r_score_ce_bf16_bwd_rows(L._stream(), L._p(prec_b), L._p(table_b), L._p(tgt), L._p(log_mask), L._p(lse), L._p(loss_ws), loss_scale, L._p(scale_dev), L._p(d_prec),
                                                L._p(ws), R, N1, E, ranges), 'a4r_score_ce_bf16_bwd_rows')
    if d_table is not None:
        assert d_table.dtype == torch.float32 and d_table.dim() == 2 and d_table.stride(1) == 1 and d_table.shape[0] >= N1
        L._check(L.lib().a4r_score_ce_bf16_bwd_items(L._stream(), L._p(prec_b), L._p(table_b), L._p(tgt), L._p(log_mask), L._p(lse), L._p(loss_ws), loss_scale, L._p(scale_dev), L._p(d_table),
                                                 d_table.stride(0), R, N1, E), 'a4r_score_ce_bf16_bwd_items')
