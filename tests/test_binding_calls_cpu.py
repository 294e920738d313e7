"""CPU: every wrapper of adapter4rec_amd/_lib.py executes its own `lib().a4r_*(...)` line against a recorder that stands in for the loaded library
(the wrappers themselves are NOT replaced, unlike tests/sim_lib.py).  The recorder holds each call against the binding's signature table: the
number of arguments, every argument's conversion by that position's declared type, and that every address is one of the case's tensors.  No
values are computed: the tensors are the smallest host tensors the wrappers' own assertions accept."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

import sim_lib
from adapter4rec_amd import _lib as L

BF, U8, I32, I64 = torch.bfloat16, torch.uint8, torch.int32, torch.int64
RETURNS = dict(a4r_topk_ws_bytes=64, a4r_score_ce_ws_bytes=64, a4r_score_ce_ranges=1, a4r_id_index_ws_ints=16, a4r_lora_bwd_fused_ws_floats=64,
               a4r_gemm_variant=2, a4r_gemm_tail_max=3, a4r_version=L.ABI_VERSION)         # the size and count queries; everything else: status 0
OWN_WORKSPACE = dict(a4r_topk_items=7, a4r_lora_bwd_fused=26)     # the pointer position of a scratch tensor the wrapper allocates itself
NO_WRAPPER = ['a4r_version']                                      # exports without a wrapper: lib() itself calls it when it loads the library
BIG_SEED = 2 ** 63 + 12345
# wrappers tests/sim_lib.py does not restate (the engine tests that need them bring their own numpy restatement or run on the GPU only); a new
# wrapper goes either into the stand-in or into this list
NO_STAND_IN = ['adamw_step', 'encoder_layer_bwd', 'encoder_layer_fwd', 'gemm_rows_256', 'gemm_tail_max', 'gemm_tail_plan', 'gemm_variant', 'grad_sumsq',
               'id_grad_sum', 'id_index', 'id_index_ws_ints', 'id_sample', 'score_ce_bwd', 'score_ce_fwd', 'score_ce_ranges', 'score_ce_ws_bytes',
               'topk_items', 'topk_ws_bytes']


def struct_pointers(s):
    for name, t in s._fields_:
        if t is ctypes.c_void_p:
            yield getattr(s, name)
        elif issubclass(t, ctypes.Array) and issubclass(t._type_, ctypes.Structure):
            for e in getattr(s, name):
                yield from struct_pointers(e)


class Recorder:
    """Stands where the CDLL object stands: `rec.a4r_x(*args)` checks the call against L.SIGNATURES['a4r_x']."""

    def __init__(self):
        self.calls, self.known = {}, set()

    def tensor(self, *shape, dtype=torch.float32):
        x = torch.zeros(*shape, dtype=dtype)
        self.known.add(x.data_ptr())
        return x

    def __getattr__(self, name):
        if not name.startswith('a4r_'):
            raise AttributeError(name)
        restype, argtypes = L.SIGNATURES[name]

        def call(*args):
            assert len(args) == len(argtypes), f'{name}: {len(args)} arguments for {len(argtypes)} parameters'
            for i, (t, a) in enumerate(zip(argtypes, args)):
                t.from_param(a)                                      # what a foreign function with this argtype does first: raises if refused
                if t is ctypes.c_void_p:
                    if isinstance(a, int) and a != 0 and OWN_WORKSPACE.get(name) != i:
                        assert a in self.known, f'{name}: argument {i} is no tensor of this case'
                elif hasattr(t, 'contents'):                         # POINTER(mirror): the addresses inside the struct(s)
                    items = a if isinstance(a, ctypes.Array) else [a._obj]
                    assert all(p is None or p in self.known for s in items for p in struct_pointers(s)), f'{name}: a stray address in argument {i}'
                else:
                    assert not isinstance(a, (ctypes._SimpleCData, torch.Tensor)) and a not in self.known, f'{name}: argument {i} = {a!r} is an address'
            self.calls[name] = self.calls.get(name, 0) + 1
            return RETURNS.get(name, 0)
        return call


@pytest.fixture
def rec(monkeypatch):
    r = Recorder()
    monkeypatch.setattr(L, '_lib', r)
    monkeypatch.setattr(L, 'require_gpu', lambda *tensors: None)
    monkeypatch.setattr(L, '_stream', lambda: 0)
    monkeypatch.setattr(L, '_lora_ws', {})
    return r


def test_every_wrapper_marshals_what_the_header_declares(rec):
    t = rec.tensor
    M, H = 128, 64
    act = lambda dtype=BF: t(M, H, dtype=dtype)
    vec = lambda n=H: t(n)

    # ---- GEMMs
    L.gemm_nt(act(), t(H, H, dtype=BF), act())
    L.gemm_nt(act(), t(H, H, dtype=BF), act(), bias=vec(), C2=act(), R1=act(), R2=act(), Pre=act(), act=L.ACT_GELU, dact=L.DACT_MUL, alpha=2, drop_p=0.1,
              drop_site=3, drop_seed=BIG_SEED, M=np.int64(M), drop_first=True, c2_deriv=True, scale_a=vec(M), scale_b=vec(), c_scale_out=vec(M), q8_tiled=True)
    assert L.gemm_variant(-1) == 2 and L.gemm_tail_max(-1) == 3 and L.gemm_tail_plan(256, 256) == (0, 0) and L.gemm_rows_256(256, 256) == 0
    X, Y, Cacc = act(), act(), t(H, H)
    L.gemm_tn(X, Y, Cacc)
    L.gemm_tn(X, Y, Cacc, M=np.int64(64))                                   # an index type that is not int
    L.gemm_tn_bias(X, Y, Cacc, vec(), M=np.int32(64))
    L.gemm_tn_multi([(X, Y, Cacc, None), (act(), act(), t(H, H), vec())])
    L.gemm_tn2(X, Y, Cacc, act(), act(), t(H, H))
    L.gemm_tn2(X, Y, Cacc, act(), act(), t(H, H), M=64, xsum1=vec(), xsum2=vec())
    L.colsum(X, vec())
    L.colsum(X, vec(), M=64)

    # ---- adapter + LayerNorm, LayerNorm
    Wd, Wu, g, b, st = t(64, H, dtype=BF), t(H, 64, dtype=BF), vec(), vec(), t(M, 2)
    A = act()
    L.adapter_ln_fwd(A, A, None, Wd, vec(64), Wu, vec(), g, b, 1e-12, L.ACT_GELU, t(M, 64, dtype=BF), t(M, 64, dtype=BF), None, act(), st)
    L.adapter_ln_fwd(A, A, act(), Wd, vec(64), Wu, vec(), g, b, 1e-12, L.ACT_GELU, t(M, 64, dtype=BF), t(M, 64, dtype=BF), act(), act(), st, M=64,
                     y8=act(U8), ys=vec(M), res32=act(torch.float32), y32=act(torch.float32), frag=(t(64 * H, dtype=BF), t(64 * H, dtype=BF)))
    L.adapter_ln_fwd(A, A, act(), Wd, vec(64), Wu, vec(), g, b, 1e-12, L.ACT_GELU, t(M, 64, dtype=BF), t(M, 64, dtype=BF), None, None, st, y8=act(U8),
                     ys=vec(M), res32=t(M, H // 2, dtype=torch.int8), y32=t(M, H // 2, dtype=torch.int8))
    bwd = lambda **kw: L.adapter_ln_bwd(act(), act(), st, g, kw.pop('dres', None), t(M, 64, dtype=BF), L.ACT_GELU, t(64, H, dtype=BF), t(H, 64, dtype=BF),
                                        True, act(), t(M, 64, dtype=BF), act(), **kw)
    bwd()
    bwd(dres=act(), dgamma=vec(), dbeta=vec(), dbias=vec(), M=64, drop_p=0.1, drop_site=5, drop_seed=BIG_SEED, dbd=vec(64), bias_total=True, beta_y=vec(),
        frag=(t(64 * H, dtype=BF), t(64 * H, dtype=BF)))
    L.ln_fwd_sum(act(), act(), g, b, 1e-12, act(), st)
    L.ln_fwd_sum(act(), None, g, b, 1e-12, act(), st, M=64, res32=act(torch.float32), sum_out=act(), sum32=act(torch.float32), y32=act(torch.float32))
    L.ln_fwd(act(), g, b, 1e-12, act(), st)
    L.ln_fwd(act(), g, b, 1e-12, act(), st, M=64, add=t(4, H), drop_p=0.1, drop_site=1, drop_seed=BIG_SEED)
    L.ln_fwd(act(), g, b, 1e-12, None, st, y8=act(U8), ys=vec(M))                       # the fp8 branch, y absent / present
    L.ln_fwd(act(), g, b, 1e-12, act(), st, add=t(4, H), y8=act(U8), ys=vec(M))
    L.ln_bwd(act(), act(), st, g, act())
    L.ln_bwd(act(), act(), st, g, act(), M=64, add=t(4, H), dgamma=vec(), dbeta=vec(), dbias=vec(), dres=act(), drop_p=0.1, drop_site=1, drop_seed=BIG_SEED,
             dv2=act(), drop2_p=0.2, drop2_site=2, drop2_seed=BIG_SEED + 1)
    L.quant_rows_fp8(act(), act(U8), vec(M))
    L.dropout_apply(act(), act(), 0.1, 7, BIG_SEED)
    L.act_bwd_f32(t(8, H), t(8, H), t(8, H), L.ACT_GELU)

    # ---- attention, SASRec block, encoder layer (n_items = 2, S = 4)
    n, S, nh, dh = 2, 4, 2, 32
    qkv, ctx = t(n * S, 3 * H), t(n * S, H)
    geo = (n, S, nh, dh, 0, H, 2 * H)
    L.attn_fwd(qkv, ctx, None, *geo, False, 0.125, -1e9)
    L.attn_fwd(qkv, ctx, t(n, S), *geo, True, 0.125, -1e9, drop_p=0.1, drop_site=2, drop_seed=BIG_SEED, offsets=t(n + 1, dtype=I32))
    L.attn_bwd(qkv, t(n * S, H), t(n * S, 3 * H), None, *geo, False, 0.125, -1e9)
    L.attn_bwd(qkv, t(n * S, H), t(n * S, 3 * H), t(n, S), *geo, True, 0.125, -1e9, drop_p=0.1, drop_site=2, drop_seed=BIG_SEED, offsets=t(n + 1, dtype=I32))
    L.attn_long_fwd(qkv, ctx, t(n * nh * S), *geo, 0.125)
    L.attn_long_fwd(qkv, ctx, t(n * nh * S), *geo, 0.125, drop_p=0.1, drop_site=2, drop_seed=BIG_SEED, key_mask=t(n, S), causal=True)
    L.attn_long_bwd(qkv, ctx, t(n * S, H), t(n * S, 3 * H), t(n * nh * S), t(n * nh * S), *geo, 0.125)
    L.attn_long_bwd(qkv, ctx, t(n * S, H), t(n * S, 3 * H), t(n * nh * S), t(n * nh * S), *geo, 0.125, drop_p=0.1, drop_site=2, drop_seed=BIG_SEED,
                    key_mask=t(n, S), causal=True)
    desc = {k: vec() for k in L.SasrecBlock._PTRS}
    desc.update(E=64, n_heads=2, F=256, d=16, ldwu=16, ldg_d=64, ldg_u=16, act=1, inner_res=1, eps=1e-8, mask_neg=-1e9, drop_attn=0.1, drop_hidden=0.1,
                drop_site=4, drop_seed=BIG_SEED, mode=1, ln3_g=vec(), ln3_b=None, g_ln3_g=None, g_ln3_b=vec())
    L.sasrec_block(desc, t(n * S, 64), t(n, S), t(n * S, 64), n, S, True)
    L.sasrec_block(desc, t(n * S, 64), t(n, S), t(n * S, 64), n, S, False, dy=t(n * S, 64))
    layer = L.EncoderLayer(M=M, H=H, drop_seed=BIG_SEED, wqkv=t(3 * H, H, dtype=BF).data_ptr())
    layer.ad[1].wd = Wd.data_ptr()
    L.encoder_layer_fwd(layer, act(), act(), act())
    L.encoder_layer_bwd(layer, act(), act(), act(), None)
    L.encoder_layer_bwd(layer, act(), act(), act(), act())

    # ---- image and text input side
    L.patchify(t(n, 3, 16, 16), t(n * 4, 192, dtype=BF), 8)
    L.patchify(t(n, 16, 16, 3, dtype=U8), t(n * 2, 192, dtype=BF), 8, keep_idx=t(n, 2, dtype=I32))
    L.mae_keep_indices(t(n, 2, dtype=I32), 4)
    L.mae_keep_indices(t(n, 2, dtype=I32), 4, noise=t(n, 4), seed=BIG_SEED, site=9)
    L.resample_u8(t(2, 4, 3, dtype=U8), t(2, 2, 3, dtype=U8), t(4, dtype=I32), t(2, 3, dtype=I32), 2, 4, 2, 3)
    L.vit_assemble(t(n * 4, H, dtype=BF), vec(), t(5, H), t(n * 5, H, dtype=BF), n, 4)
    L.vit_assemble(t(n * 4, H, dtype=BF), vec(), t(5, H), t(n * 6, H, dtype=BF), n, 4, keep_idx=t(n, 4, dtype=I32), tokens_out=6)
    ids = t(n, 2 * S, dtype=I64)
    L.embed_ln(ids, t(10, H), t(S, H), vec(), g, b, 1e-12, t(n * S, H, dtype=BF), n, S)
    L.embed_ln(ids, t(10, H), t(S + 2, H), vec(), g, b, 1e-12, t(n * S, H, dtype=BF), n, S, roberta=True, pad_id=1, drop_p=0.1, drop_site=1,
               drop_seed=BIG_SEED, pre_out=t(n * S, H, dtype=BF), stats_out=t(n * S, 2), key_mask_out=t(n, S))
    L.embed_bwd(ids, t(n * S, H, dtype=BF), None, None, n, S)
    L.embed_bwd(ids, t(n * S, H, dtype=BF), t(10, H), t(S + 2, H), n, S, roberta=True, pad_id=1)

    # ---- rows, ID tower
    src, dst = t(n * S, H, dtype=BF), t(n, H, dtype=BF)
    L.gather_rows(src, dst, n, S)
    L.scatter_rows(dst, src, n, S)
    L.scatter_rows_fill(dst, src, n, S, n * S)
    L.rows_idx_copy(src, dst, t(n, dtype=I32), n)
    L.rows_idx_copy(dst, src, t(n, dtype=I32), n, scatter=True)
    L.zero(t(16))
    assert L.id_index_ws_ints(8, 10) == 16
    rows, slots, ptr, uniq, n_uniq, err = (t(k, dtype=I32) for k in (8, 8, 9, 8, 1, 1))
    L.id_index(t(8, dtype=I64), 10, rows, slots, ptr, uniq, n_uniq, err, t(16, dtype=I32))
    L.id_grad_sum(t(8, H), slots, ptr, uniq, n_uniq, 8, t(11, H))
    L.id_sample(t(3, S, dtype=I32), t(2, dtype=I32), 10, BIG_SEED, 1, True, t(2, S, 2, dtype=I64), t(2, S - 1), err)
    L.id_sample(t(3, S, dtype=I32), t(2, dtype=I32), np.int64(10), -1, np.int32(1), False, t(2, S, 2, dtype=I64), t(2, S - 1), err)

    # ---- parameter side
    W, dstW, dstT = t(H, H), t(H, H, dtype=BF), t(H, H, dtype=BF)
    L.lora_merge(W, t(8, H), t(H, 8), 0.5, dstW, dstT, 8)
    L.lora_merge(W, None, None, 0.0, dstW, dstT, 0)
    tab = L.lora_table([(W, t(8, H), t(H, 8), 0.5, dstW, dstT, 8), (W, None, None, 0.0, dstW, dstT, 0)], 'cpu')
    rec.known.add(tab[0].data_ptr())
    L.lora_merge_batch(tab)
    w8 = lambda: t(8, H, dtype=BF)
    L.lora_bwd_fused(t(16, H, dtype=BF), t(16, H, dtype=BF), t(16, H, dtype=BF), w8(), w8(), w8(), w8(), 0.5, 0.25, t(8, H), t(8, H), t(H, 8), t(H, 8),
                     vec(), None, 16)
    L.lora_bwd_fused(t(16, H, dtype=BF), t(16, H, dtype=BF), t(16, H, dtype=BF), w8(), w8(), w8(), w8(), 0.5, 0.25, t(8, H), t(8, H), t(H, 8), t(H, 8),
                     None, vec(), 16, rank_rows=16)
    table = t(80, dtype=U8)
    L.phm_build(t(16), table, 1, t(16))
    L.phm_bwd(t(16), table, 1, t(16))
    L.unpack_add(t(16), table, 1, 16)
    L.pack_matrices(t(16), table, 1, 16, L.BF16)
    p, seg = (t(8), t(8), t(8), t(8)), (t(1, dtype=I32), t(1, dtype=I32))
    L.adam_step(*p, *seg, t(1), 1)
    L.adam_step(*p, *seg, t(1), np.int64(2), beta1=0.8, beta2=0.9, eps=1e-6, grad_scale=0.5)
    parts = t(L.GRAD_NORM_PARTS, dtype=torch.float64)
    L.grad_sumsq(p[1], parts, grad_scale=0.5)
    L.adamw_step(*p, *seg, t(1), t(1), 1)
    L.adamw_step(*p, *seg, t(1), t(1), np.int64(2), decoupled=False, partials=parts, max_norm=1.0, norm_out=t(1))

    # ---- heads and evaluation
    B, Ls, E = 2, 3, 64
    emb, prec, lm, pos, neg, lw = t(B, Ls, 2, E), t(B * (Ls - 1), E), t(B, Ls - 1), t(B, Ls - 1), t(B, Ls - 1), t(4)
    L.score_bce_fwd(emb, prec, lm, pos, neg, lw, B, Ls, E, False)
    L.score_bce_bwd(emb, prec, lm, pos, neg, lw, 1.0, t(B * (Ls - 1), E), t(B, Ls, 2, E), B, Ls, E, True)
    L.score_bce_bwd(emb, prec, lm, pos, neg, lw, 1.0, t(B * (Ls - 1), E), t(B, Ls, 2, E), B, Ls, E, True, scale_dev=t(1))
    L.emb_grad_add_inputs(prec, emb, B, Ls, E)
    L.take_inputs(emb, prec, B, Ls, E)
    R, N1 = 4, 9
    tbl, tgt, mask, lse = t(N1, E), t(R, dtype=I32), t(R), t(R)
    assert L.score_ce_ranges(R, N1) == 1 and L.score_ce_ws_bytes(R, N1, E) == 64 and L.score_ce_ws_bytes(R, N1, E, ranges=2) == 64
    L.score_ce_fwd(prec, tbl, tgt, mask, lse, t(R), lw, R, ws=t(64, dtype=U8))
    L.score_ce_fwd(prec, tbl, tgt, mask, lse, t(R), lw, np.int64(R), ranges=2, ws=t(64, dtype=U8))
    before = dict(rec.calls)
    L.score_ce_bwd(prec, tbl, tgt, mask, lse, lw, 1.0, t(R, E), None, R, ws=t(64, dtype=U8))                # the rows launch alone
    assert rec.calls['a4r_score_ce_bwd_rows'] == 1 and 'a4r_score_ce_bwd_items' not in rec.calls and before.keys() | {'a4r_score_ce_bwd_rows'} == rec.calls.keys()
    L.score_ce_bwd(prec, tbl, tgt, mask, lse, lw, 1.0, None, t(N1, E), R)                                    # the items launch alone
    assert rec.calls['a4r_score_ce_bwd_rows'] == 1 and rec.calls['a4r_score_ce_bwd_items'] == 1
    L.score_ce_bwd(prec, tbl, tgt, mask, lse, lw, 1.0, t(R, E), t(N1, E), R, ranges=2, scale_dev=t(1), ws=t(64, dtype=U8))
    assert L.topk_ws_bytes(R, N1, 3) == 64
    L.topk_items(prec, tbl, t(R + 1, dtype=I32), t(1, dtype=I32), 3, t(R, 3, dtype=I32), t(R, 3))
    L.eval_rank(prec, tbl, t(R, dtype=I32), t(R + 1, dtype=I32), t(1, dtype=I32), t(R, dtype=I32))

    # nothing is left out: every export was reached through its wrapper, the launches (a `stream` parameter) and the host-side queries alike
    assert sorted(set(rec.calls) | set(NO_WRAPPER)) == sorted(L.SIGNATURES) and not set(rec.calls) & set(NO_WRAPPER)


def test_index_types_flags_and_large_seeds_convert(rec):
    """What the explicit constructors used to accept still converts: anything with __index__ for an integer, a bool for a flag, a seed above 2^63."""
    for t, v, want in ((ctypes.c_int, np.int64(128), 128), (ctypes.c_int, np.int32(7), 7), (ctypes.c_int, True, 1), (ctypes.c_int64, np.int64(2 ** 40), 2 ** 40),
                       (ctypes.c_uint64, BIG_SEED, BIG_SEED), (ctypes.c_uint64, 2 ** 64 - 1, 2 ** 64 - 1), (ctypes.c_uint32, np.int64(7001), 7001),
                       (ctypes.c_float, 1, 1.0), (ctypes.c_float, np.float32(0.5), 0.5), (ctypes.c_long, np.int64(3), 3)):
        f = ctypes.CFUNCTYPE(t, t)(lambda x: x)                      # a real foreign call through the declared type
        assert f(v) == want, (t, v)
    assert L.gemm_tail_max(True) == 3 and L.gemm_rows_256(np.int64(256), np.int32(256)) == 0
    assert rec.calls == dict(a4r_gemm_tail_max=1, a4r_gemm_rows_256=1)


def test_a_float_for_an_int_is_refused_not_truncated(rec):
    X, Y, Cacc = rec.tensor(128, 64, dtype=BF), rec.tensor(128, 64, dtype=BF), rec.tensor(64, 64)
    with pytest.raises((TypeError, ctypes.ArgumentError)):
        L.gemm_tn(X, Y, Cacc, M=128.0)
    with pytest.raises((TypeError, ctypes.ArgumentError)):
        L.gemm_rows_256(256.5, 256)
    assert not rec.calls


def test_layernorm_operands_read_through_a_bare_pointer_are_checked(rec):
    """gamma, beta, add and stats reach the LayerNorm kernels as bare pointers: read as contiguous, add at leading dimension H, stats as [M, 2].  A
    strided view, another dtype, a table of another width or too few rows of stats are refused by the wrapper, not silently misread."""
    t = rec.tensor
    M, H = 16, 64
    act, g, b, st = (lambda: t(M, H, dtype=BF)), t(H), t(H), t(M, 2)
    bad_vec = [t(2 * H)[::2], t(H, dtype=BF), t(H // 2)]
    bad_stats = [t(M, 4)[:, :2], t(M - 1, 2), t(2, M).t(), t(M, 2, dtype=BF), t(2 * M)]
    bad_add = [t(4, 2 * H)[:, :H], t(4, H, dtype=BF), t(4, H // 2), t(4 * H), t(8, H)[::2]]
    calls = []
    for v in bad_vec:
        calls += [lambda v=v: L.ln_fwd(act(), v, b, 1e-12, act(), st), lambda v=v: L.ln_fwd(act(), g, v, 1e-12, act(), st),
                  lambda v=v: L.ln_fwd(act(), g, v, 1e-12, None, st, y8=act().view(U8)[:, :H], ys=t(M)),
                  lambda v=v: L.ln_bwd(act(), act(), st, v, act()), lambda v=v: L.ln_fwd_sum(act(), act(), v, b, 1e-12, act(), st),
                  lambda v=v: L.ln_fwd_sum(act(), act(), g, v, 1e-12, act(), st)]
    for s_ in bad_stats:
        calls += [lambda s_=s_: L.ln_fwd(act(), g, b, 1e-12, act(), s_), lambda s_=s_: L.ln_bwd(act(), act(), s_, g, act()),
                  lambda s_=s_: L.ln_fwd_sum(act(), act(), g, b, 1e-12, act(), s_)]
    for a in bad_add:
        calls += [lambda a=a: L.ln_fwd(act(), g, b, 1e-12, act(), st, add=a), lambda a=a: L.ln_bwd(act(), act(), st, g, act(), add=a)]
    calls.append(lambda: L.ln_fwd(act(), g, b, 1e-12, act(), t(M, 2), M=M + 1))          # M rows asked of stats that has fewer
    for f in calls:
        with pytest.raises(AssertionError):
            f()
    assert not rec.calls
    rows, half = t(8, H)[2:6], t(2 * H)[H:]                                              # contiguous slices (a table's rows, a flat buffer's tail): accepted
    rec.known.update((rows.data_ptr(), half.data_ptr()))
    L.ln_fwd(act(), g, b, 1e-12, act(), st, add=rows)
    L.ln_fwd(act(), g, b, 1e-12, act(), None)                                            # stats are optional in a4r_ln_fwd
    L.ln_bwd(act(), act(), t(M + 3, 2), half, act(), M=M)
    assert rec.calls == dict(a4r_ln_fwd=2, a4r_ln_bwd=1)


def test_the_loaded_library_enforces_the_table():
    """The same on the real library's host-side queries (no GPU needed): lib() installed the table, so a float, a missing argument and a foreign struct
    raise instead of reaching the C code (a surplus argument ctypes lets through on a cdecl function: the recorder above counts them)."""
    lib = L.lib()
    assert all(getattr(lib, name).argtypes == argtypes and getattr(lib, name).restype is restype for name, (restype, argtypes) in L.SIGNATURES.items())
    assert lib.a4r_gemm_rows_256(0, 0) == 0
    for bad in ((256.0, 256), (256,)):
        with pytest.raises((TypeError, ctypes.ArgumentError)):
            lib.a4r_gemm_rows_256(*bad)
    with pytest.raises(ctypes.ArgumentError):                       # byref of the wrong struct (never reaches a4r_gemm_nt)
        lib.a4r_gemm_nt(None, ctypes.byref(L.AttnArgs()))


def test_the_stand_in_restates_every_wrapper_signature_exactly():
    """tests/sim_lib.py replaces the wrappers in the engine tests: every function both modules define (not merely re-exported) has the same
    parameter names, order and defaults, and every public wrapper is either restated there or listed above."""
    own = lambda mod: {n: f for n, f in vars(mod).items() if inspect.isfunction(f) and f.__module__ == mod.__name__}
    real, sim = own(L), own(sim_lib)
    shared = sorted(set(real) & set(sim))
    assert len(shared) >= 48
    for name in shared:
        assert inspect.signature(real[name]) == inspect.signature(sim[name]), name
    reexported = {n for n in real if getattr(sim_lib, n, None) is real[n]}
    assert sorted(n for n in real if not n.startswith('_') and n not in sim and n not in reexported) == sorted(NO_STAND_IN)
