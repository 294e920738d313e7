"""IdRecEngine: the IDRec baseline of the image path (Downstream/CV/model/model.py:33-35, 55-58 with use_modal=False) -- the SASRec / CPC
user tower fed by a learned item-ID table instead of an item encoder.

Forward: a4r_id_index turns the batch's slot ids into the int32 rows a4r_rows_idx_copy gathers the table with, plus the inverted index (every
distinct id's slots in slot order); the user tower is TransRecEngine's, the head its BCE head (--loss bce) or the softmax cross-entropy over the
whole table (--loss ce: a4r_score_ce_*, whose item-side gradient is dense and goes straight into the table's gradient).  Backward: TransRecEngine's head + user-tower half,
then a4r_id_grad_sum adds each listed row's gradient into the table's slice of the flat gradient buffer in a fixed order (no float atomics:
the table gradient is a function of the batch alone).  The table lives in flat_p as fp32 and the forward reads that parameter view directly.
"""
import torch

from . import _lib as L
from .engine import TransRecEngine, pad_to


def loss_flag(args, arch, use_modal):
    """args.loss ('bce' when absent) after the checks of --loss ce: it needs the ID table as its candidate set and the SASRec user tower."""
    loss = getattr(args, 'loss', 'bce') or 'bce'
    if loss not in ('bce', 'ce'):
        raise ValueError(f"--loss must be 'bce' or 'ce', got {loss!r}")
    if loss == 'ce' and use_modal:
        raise NotImplementedError('--loss ce with an item encoder (--item_tower modal): the full-softmax head needs the candidate set to be '
                                  'the ID table itself (--item_tower id)')
    if loss == 'ce' and arch == 'cpc':
        raise NotImplementedError('--loss ce with --arch cpc: the full-softmax head is built for the SASRec user tower only')
    return loss


def ce_dtype_flag(args, loss):
    """args.ce_dtype ('fp32' when absent): the number format of the cross-entropy head's two products.  --compute_dtype does not imply it."""
    ce_dtype = getattr(args, 'ce_dtype', 'fp32') or 'fp32'
    if ce_dtype not in ('fp32', 'bf16'):
        raise ValueError(f"--ce_dtype must be 'fp32' or 'bf16', got {ce_dtype!r}")
    if ce_dtype == 'bf16' and loss != 'ce':
        raise NotImplementedError('--ce_dtype bf16 without --loss ce: it selects the number format of the full-softmax head, the BCE head has one')
    return ce_dtype


class IdRecEngine(TransRecEngine):
    MULTI_ATTR = False

    def __init__(self, model, args, arch='sasrec', dtype='bf16', phm_owner=None):
        if dtype == 'fp8':
            raise NotImplementedError('--compute_dtype fp8 with --item_tower id: the ID tower has no backbone GEMM to quantise')
        self.loss = loss_flag(args, arch, False)
        self.ce_dtype = ce_dtype_flag(args, self.loss)
        super().__init__(model, args, arch=arch, dtype=dtype, phm_owner=phm_owner)
        self._err_pending, self._err_free = [], []           # (pinned host word, event) per step not yet checked; spare words

    def _build_item_tower(self):
        w = self.model.id_embedding.weight
        self.item_num = w.shape[0] - 1
        if w.shape[1] != self.E or self.E % 4:
            raise NotImplementedError(f'ID table width {w.shape[1]} (embedding_dim {self.E}, a multiple of 4)')
        if self.ce_dtype == 'bf16' and self.E not in L.SCORE_CE_BF16_E:
            raise NotImplementedError(f'--ce_dtype bf16 with embedding_dim {self.E}: a4r_score_ce_bf16_* serves the widths {L.SCORE_CE_BF16_E}')
        if self.loss == 'ce' and self.E not in L.SCORE_CE_E:
            raise NotImplementedError(f'--loss ce with embedding_dim {self.E}: a4r_score_ce_* serves the widths {L.SCORE_CE_E}')
        self.H = self.E
        self.bert_blocks, self.bert_kads, self.cls_only, self.train_emb, self.prompt_n = [], [], False, False, 0
        self.table = w.data if w.requires_grad else self._f32(w)          # (trainable: the fp32 view into flat_p, never repacked)
        self.g_table = self.grad_view(w)

    # ------------------------------------------------------------------ index + gather
    def _check_ids(self, ids):
        """Host ids are range-checked before anything is enqueued (nn.Embedding raises IndexError); device ids are taken as they are and an
        out-of-range one is counted by a4r_id_index (reported by a later step, see _raise_pending)."""
        if not ids.is_cuda and ids.numel():
            lo, hi = int(ids.min()), int(ids.max())
            if lo < 0 or hi > self.item_num:
                raise IndexError(f'index out of range in self: item ids must lie in [0, {self.item_num}], got [{lo}, {hi}]')
        return ids.to(self.dev, non_blocking=True)

    def _raise_pending(self):
        """The error words of earlier steps whose copies to pinned host memory have landed (queried, never waited for)."""
        while self._err_pending and (self._err_pending[0][1] is None or self._err_pending[0][1].query()):
            host, _ = self._err_pending.pop(0)
            bad = int(host[0])
            self._err_free.append(host)
            if bad:
                raise IndexError(f'index out of range in self: {bad} item ids of an earlier batch outside [0, {self.item_num}] (read as row 0)')

    def _post_err(self, err):
        """Copy this step's error word to pinned host memory behind the step's work; a later step reads it once the copy has landed."""
        if not err.is_cuda:                         # (host-logic tests: a CPU stand-in of the library)
            self._err_pending.append((err.clone(), None))
            return
        host = self._err_free.pop() if self._err_free else torch.zeros(1, dtype=torch.int32).pin_memory()
        host.copy_(err, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        self._err_pending.append((host, ev))

    def _index(self, ids, n):
        """a4r_id_index into this engine's buffers -> dict of device tensors (rows, slots, ptr, uniq, n_uniq, err)."""
        i32 = torch.int32
        ix = dict(rows=self._buf('id.rows', n, 1, i32).view(-1), slots=self._buf('id.slots', n, 1, i32).view(-1),
                  ptr=self._buf('id.ptr', n + 1, 1, i32).view(-1), uniq=self._buf('id.uniq', n, 1, i32).view(-1),
                  n_uniq=self._buf('id.nu', 1, 1, i32).view(-1), err=self._buf('id.err', 1, 1, i32).view(-1))
        ws = self._buf('id.ws', L.id_index_ws_ints(n, self.item_num), 1, i32).view(-1)
        L.id_index(ids, self.item_num, ix['rows'], ix['slots'], ix['ptr'], ix['uniq'], ix['n_uniq'], ix['err'], ws)
        return ix

    def _gather(self, rows, n, out):
        """out[r] = table[rows[r]], r < n (a4r_rows_idx_copy)."""
        L.rows_idx_copy(self.table, out, rows, n)

    # ------------------------------------------------------------------ public entry points
    @torch.no_grad()
    def encode_items(self, ids):
        """item ids (any integer tensor) -> fp32 [n, E]: the table rows."""
        flat = ids.reshape(-1)
        n = flat.numel()
        out = torch.zeros(n, self.E, dtype=torch.float32, device=self.dev)
        if n == 0:
            return out
        if flat.is_cuda:
            flat = flat.to(torch.int32)
            if not bool(((flat >= 0) & (flat <= self.item_num)).all()):
                raise IndexError(f'index out of range in self: item ids must lie in [0, {self.item_num}]')
        else:
            self._check_ids(flat)
            flat = flat.to(torch.int32).to(self.dev)
        self._gather(flat.contiguous(), n, out)
        return out

    def table_copy(self):
        """The whole table [item_num + 1, E] fp32 (evaluation's item embeddings, data_utils/metrics.py:52-63)."""
        out = torch.empty(self.item_num + 1, self.E, dtype=torch.float32, device=self.dev)
        out.copy_(self.table)
        return out

    def train_forward(self, sample_items, log_mask):
        """sample_items: flat int64 slot ids [B * L * 2] (the reference's .view(-1) batch) on the host or the device; log_mask [B, L-1]
        -> loss (0-d fp32 device tensor)."""
        self._raise_pending()
        self.host_log_mask = self.host_lens = self.host_max_tokens = None          # (hints of the item encoders: nothing to skip here)
        ids = sample_items.reshape(-1)
        if ids.dtype != torch.int64:
            ids = ids.long()
        ids = self._check_ids(ids).contiguous()
        L.require_gpu(ids, log_mask)
        train = self.model.training
        n_full = ids.numel()
        B = n_full // (2 * self.Lseq)
        assert B * 2 * self.Lseq == n_full and tuple(log_mask.shape) == (B, self.Lseq - 1), (n_full, tuple(log_mask.shape))
        lm = log_mask.float().contiguous()
        self.pack_trainables()
        self.step_count += 1
        seed = (self.seed * 1000003 + self.step_count) & 0xFFFFFFFFFFFF
        E = self.E
        Mu = pad_to(B * (self.Lseq - 1), 128)
        if self._saved_sas is None or self._saved_Mu != Mu:
            self._saved_sas = [self._block_bufs(f'sas.{j}', b, Mu, False) for j, b in enumerate(self.sas_blocks)]
            self._saved_Mu = Mu
        ix = self._index(ids, n_full)
        # every slot is gathered (pad slots read row 0, as nn.Embedding does); the rows past n_full stay zero
        emb = self._buf_tail0('emb_full', pad_to(n_full, 128), E, torch.float32, n_full)
        self._gather(ix['rows'], n_full, emb)
        xin = self._buf('sxin', Mu, E, torch.float32)
        L.take_inputs(emb, xin, B, self.Lseq, E)
        prec, Mu = self._user_forward(xin, lm, B, train, seed, self._saved_sas)
        ws = self._buf('lossws', 1, 4, torch.float32)
        if self.loss == 'ce':
            return self._ce_forward(B, n_full, Mu, seed, train, lm, emb, prec, xin, ws, ix)
        pos = self._buf('pos', B, self.Lseq - 1, torch.float32)
        neg = self._buf('neg', B, self.Lseq - 1, torch.float32)
        L.zero(ws)
        L.score_bce_fwd(emb, prec, lm, pos, neg, ws, B, self.Lseq, E, self.arch == 'cpc')
        self._post_err(ix['err'])
        self._ctx = dict(B=B, n_items=n_full, n_full=n_full, M=0, Mu=Mu, seed=seed, train=train, lm=lm, emb=emb, prec=prec, xin=xin, pos=pos,
                         neg=neg, ws=ws, saved_s=self._saved_sas, ix=ix)
        return ws[0, 0].clone()

    # ------------------------------------------------------------------ --loss ce: softmax cross-entropy over the whole table
    def _ce_ws(self, R):
        """The scratch a4r_score_ce_fwd and _bwd_rows share (ranges x R x E floats, whatever the table's size)."""
        ws_bytes = L.score_ce_bf16_ws_bytes if self.ce_dtype == 'bf16' else L.score_ce_ws_bytes
        return self._buf('ce.ws', ws_bytes(R, self.item_num + 1, self.E), 1, torch.uint8).view(-1)

    def _ce_cast(self, prec, R):
        """--ce_dtype bf16: this step's bf16 copies of the head's operands, made once in the forward and read again by the backward.  The
        table's copy ([item_num + 1, E] bf16, half a table) is the one buffer of the table's size the option adds."""
        table_b = self._buf('ce.table_b', self.item_num + 1, self.E, torch.bfloat16)
        prec_b = self._buf('ce.prec_b', R, self.E, torch.bfloat16)
        L.cast_bf16(self.table, table_b)
        L.cast_bf16(prec, prec_b, R * self.E)
        return prec_b, table_b

    def _ce_forward(self, B, n_full, Mu, seed, train, lm, emb, prec, xin, ws, ix):
        """The head of train_forward under --loss ce: row (b, t) is trained against every item of the table with the positive id of position
        t + 1 as its class (a4r_score_ce_fwd); the batch's sampled negatives are not read.  rows holds the range-checked slot ids."""
        T = self.Lseq - 1
        R = B * T
        tgt = self._buf('ce.tgt', R, 1, torch.int32).view(-1)
        tgt.view(B, T).copy_(ix['rows'][:n_full].view(B, self.Lseq, 2)[:, 1:, 0])
        lse = self._buf('ce.lse', R, 1, torch.float32).view(-1)
        s_tgt = self._buf('ce.s_tgt', R, 1, torch.float32).view(-1)
        cast = None
        if self.ce_dtype == 'bf16':
            cast = self._ce_cast(prec, R)
            L.score_ce_bf16_fwd(cast[0], cast[1], tgt, lm.view(-1), lse, s_tgt, ws.view(-1), R, ws=self._ce_ws(R))
        else:
            L.score_ce_fwd(prec, self.table, tgt, lm.view(-1), lse, s_tgt, ws.view(-1), R, ws=self._ce_ws(R))
        self._post_err(ix['err'])
        self._ctx = dict(B=B, n_items=n_full, n_full=n_full, M=0, Mu=Mu, seed=seed, train=train, lm=lm, emb=emb, prec=prec, xin=xin, tgt=tgt,
                         lse=lse, ws=ws, saved_s=self._saved_sas, ix=ix, ce_cast=cast)
        return ws[0, 0].clone()

    def _head_backward(self, c, grad_out, d_prec, d_emb, B):
        """--loss ce: d_prec from a4r_score_ce_bwd_rows; the target side of the head goes straight into the table's gradient (a4r_score_ce_bwd_items
        adds into the current gradient target, every row but row 0), so d_emb starts at zero and carries the user tower's input gradient alone."""
        if self.loss != 'ce':
            return super()._head_backward(c, grad_out, d_prec, d_emb, B)
        R = B * (self.Lseq - 1)
        L.zero(d_emb)
        if c['ce_cast'] is not None:
            prec_b, table_b = c['ce_cast']
            L.score_ce_bf16_bwd(prec_b, table_b, c['tgt'], c['lm'].view(-1), c['lse'], c['ws'].view(-1), 1.0, d_prec,
                                self.g_table() if self.g_table is not None else None, R, scale_dev=grad_out, ws=self._ce_ws(R))
            return
        L.score_ce_bwd(c['prec'], self.table, c['tgt'], c['lm'].view(-1), c['lse'], c['ws'].view(-1), 1.0, d_prec,
                       self.g_table() if self.g_table is not None else None, R, scale_dev=grad_out, ws=self._ce_ws(R))

    def train_backward(self, grad_out=None, into_flat_grad=False, as_list=True):
        """The shared head + user-tower backward (TransRecEngine._head_user_backward), then the table's gradient: a4r_id_grad_sum of the
        d_emb slot rows into the CURRENT gradient target (flat_g on the fused path, flat_gs under gradient accumulation)."""
        c, target, d_emb = self._head_user_backward(grad_out, into_flat_grad)
        if self.g_table is not None:
            ix = c['ix']
            L.id_grad_sum(d_emb, ix['slots'], ix['ptr'], ix['uniq'], ix['n_uniq'], c['n_full'], self.g_table())
        return self._backward_finish(target, into_flat_grad, as_list)
