"""ctypes binding of liba4r_hip.so (C ABI declared in include/a4r.h).

The library is the product's only compute path: if it is missing or a call fails this module
raises -- there is no PyTorch / CPU fallback.  Tensors are passed as raw device pointers plus
leading dimensions; kernels are enqueued on torch's current HIP stream.
"""
import ctypes as C
import importlib
import math
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('A4R_LIB_PATH') or os.path.join(_HERE, 'liba4r_hip.so')    # A4R_LIB_PATH: A/B builds (tools/), same C ABI

ABI_VERSION = 411          # = A4R_ABI_VERSION of include/a4r.h (tests/test_abi_cpu.py compares the two)
BF16, F32, FP8 = 0, 1, 2
ACT_NONE, ACT_RELU, ACT_GELU, ACT_GELU_TANH, ACT_LEAKY = 0, 1, 2, 3, 4
DACT_MUL = 15
DACT_MUL_Q8 = 14          # Pre = the uint8 derivative tensor a c2_deriv='q8' launch wrote (include/a4r.h: c2_mode 2)
Q8_OFF, Q8_STEP = 0.1289, 0.0049326
EVAL_MAX_HISTORY = 264         # A4R_EVAL_MAX_HISTORY (include/a4r.h)
ACT_BY_NAME = {'none': 0, 'relu': 1, 'RELU': 1, 'gelu': 2, 'GELU': 2, 'gelu_new': 3, 'leaky_relu': 4}

ID_SUM_CHUNK = 16          # A4R_ID_SUM_CHUNK (include/a4r.h)
TOPK_MAX_K = 256           # A4R_TOPK_MAX_K (include/a4r.h)
TOPK_E = (64, 128, 256, 512)
GRAD_NORM_PARTS = 1024     # A4R_GRAD_NORM_PARTS (include/a4r.h)
SCORE_CE_E = TOPK_E         # table widths of the cross-entropy head (a4r_score_ce_*)
SCORE_CE_MAX_RANGES = 32   # A4R_SCORE_CE_MAX_RANGES (include/a4r.h)
SAMPLE_MAX_L = 256         # a4r_id_sample: the longest sequence row (include/a4r.h)
SAMPLE_SITE = 7001         # A4R_SAMPLE_SITE (csrc/a4r_common.h): the hash site of a4r_id_sample's draws


class GemmArgs(C.Structure):
    _fields_ = [('A', C.c_void_p), ('B', C.c_void_p), ('C', C.c_void_p), ('bias', C.c_void_p), ('C2', C.c_void_p),
                ('R1', C.c_void_p), ('R2', C.c_void_p), ('Pre', C.c_void_p),
                ('M', C.c_int32), ('N', C.c_int32), ('K', C.c_int32),
                ('lda', C.c_int32), ('ldb', C.c_int32), ('ldc', C.c_int32), ('ldc2', C.c_int32),
                ('ldr1', C.c_int32), ('ldr2', C.c_int32), ('ldpre', C.c_int32),
                ('in_dtype', C.c_int32), ('out_dtype', C.c_int32), ('act', C.c_int32), ('dact', C.c_int32),
                ('drop_first', C.c_int32), ('c2_mode', C.c_int32), ('alpha', C.c_float), ('drop_p', C.c_float), ('drop_site', C.c_uint32), ('drop_seed', C.c_uint64),
                ('drop_row0', C.c_int64), ('scale_a', C.c_void_p), ('scale_b', C.c_void_p),
                ('c_fp8', C.c_int32), ('c_scale', C.c_float), ('c_scale_out', C.c_void_p), ('q8_tiled', C.c_int32)]


class AttnArgs(C.Structure):
    _fields_ = [('qkv', C.c_void_p), ('ld', C.c_int32), ('q_off', C.c_int32), ('k_off', C.c_int32), ('v_off', C.c_int32),
                ('out', C.c_void_p), ('ldo', C.c_int32), ('dout', C.c_void_p), ('dqkv', C.c_void_p), ('key_mask', C.c_void_p),
                ('n_items', C.c_int32), ('S', C.c_int32), ('n_heads', C.c_int32), ('dh', C.c_int32), ('causal', C.c_int32),
                ('dtype', C.c_int32), ('scale', C.c_float), ('mask_neg', C.c_float),
                ('drop_p', C.c_float), ('drop_site', C.c_uint32), ('drop_seed', C.c_uint64), ('offsets', C.c_void_p)]


class PackDesc(C.Structure):
    _fields_ = [('src_off', C.c_int64), ('dst', C.c_void_p), ('rows', C.c_int32), ('cols', C.c_int32),
                ('rows_pad', C.c_int32), ('cols_pad', C.c_int32), ('transpose', C.c_int32), ('dst_ld', C.c_int32)]


class PhmDesc(C.Structure):
    _fields_ = [('rule_off', C.c_int64), ('wl_off', C.c_int64), ('wr_off', C.c_int64), ('out_off', C.c_int64), ('G', C.c_void_p),
                ('ldg', C.c_int32), ('in_f', C.c_int32), ('out_f', C.c_int32), ('n', C.c_int32), ('pad_', C.c_int32)]


class LayerAdapter(C.Structure):
    """a4r_layer_adapter_t (include/a4r.h)."""
    _fields_ = [(n, C.c_void_p) for n in ('wd', 'wu', 'wdT', 'wuT', 'wd_f', 'wu_f', 'wdT_f', 'wuT_f', 'bd', 'bu', 'g_wu', 'g_wd', 'g_bu', 'g_bd')] + \
               [(n, C.c_int32) for n in ('ldg_wu', 'ldg_wd', 'act', 'pad_')]


class EncoderLayer(C.Structure):
    """a4r_encoder_layer_t (include/a4r.h): one post-LN encoder layer with serial Houlsby adapters for a4r_encoder_layer_fwd / _bwd."""
    _fields_ = [(n, C.c_int32) for n in ('M', 'H', 'F', 'n_items', 'S', 'n_heads', 'dh', 'causal')] + \
               [(n, C.c_float) for n in ('scale', 'mask_neg', 'ln_eps', 'p_attn', 'p_hidden')] + [('drop_site', C.c_uint32), ('drop_seed', C.c_uint64)] + \
               [(n, C.c_void_p) for n in ('key_mask', 'offsets', 'wqkv', 'wqkvT', 'wo', 'woT', 'wi', 'wiT', 'wo2', 'wo2T',
                                          'bqkv', 'bo', 'bi', 'bo2', 'ln1_g', 'ln1_b', 'ln2_g', 'ln2_b')] + \
               [('ad', LayerAdapter * 2)] + \
               [(n, C.c_void_p) for n in ('qkv', 'ctx', 'h1', 'v1', 'zp1', 'z1', 'u', 'upre', 'h2', 'v2', 'zp2', 'z2', 'st1', 'st2')] + \
               [('upre_q8', C.c_int32), ('q8_tiled', C.c_int32)] + \
               [(n, C.c_void_p) for n in ('x_lo', 'x1_lo', 'xout_lo', 'dv1', 'dv2', 'dzp', 'd_h', 'du', 'dx1', 'dctx', 'dqkv')] + [('lo_nibble', C.c_int32)]


class SasrecBlock(C.Structure):
    """a4r_sasrec_block_t (include/a4r.h)."""
    _PTRS = ('wqkv', 'wfc', 'w1', 'b1', 'w2', 'b2', 'ln1_g', 'ln1_b', 'ln2_g', 'ln2_b', 'wd1', 'bd1', 'wu1', 'bu1', 'wd2', 'bd2', 'wu2', 'bu2',
             'g_wd1', 'g_bd1', 'g_wu1', 'g_bu1', 'g_wd2', 'g_bd2', 'g_wu2', 'g_bu2')
    _fields_ = [(n, C.c_void_p) for n in _PTRS] + \
               [(n, C.c_int32) for n in ('E', 'n_heads', 'F', 'd', 'ldwu', 'ldg_d', 'ldg_u', 'act', 'inner_res')] + \
               [(n, C.c_float) for n in ('eps', 'mask_neg', 'drop_attn', 'drop_hidden')] + [('drop_site', C.c_uint32), ('drop_seed', C.c_uint64)] + \
               [('mode', C.c_int32)] + [(n, C.c_void_p) for n in ('ln3_g', 'ln3_b', 'g_ln3_g', 'g_ln3_b')]


class AddDesc(C.Structure):
    _fields_ = [('src', C.c_void_p), ('dst_off', C.c_int64), ('rows', C.c_int32), ('cols', C.c_int32), ('ld', C.c_int32), ('alpha', C.c_float)]


class TnProb(C.Structure):
    _fields_ = [('X', C.c_void_p), ('Y', C.c_void_p), ('C', C.c_void_p), ('xsum', C.c_void_p),
                ('ldx', C.c_int32), ('ldy', C.c_int32), ('ldc', C.c_int32), ('P', C.c_int32), ('Q', C.c_int32), ('pad_', C.c_int32)]


class LoraDesc(C.Structure):
    _fields_ = [('W', C.c_void_p), ('A', C.c_void_p), ('B', C.c_void_p), ('dst', C.c_void_p), ('dstT', C.c_void_p),
                ('scaling', C.c_float), ('ld', C.c_int32), ('ldT', C.c_int32), ('out_f', C.c_int32), ('in_f', C.c_int32), ('r', C.c_int32)]


# The C boundary, declared once: name -> (restype, argtypes) for every export of include/a4r.h, installed by lib().  ctypes then checks the
# number and the kind of every argument of every call (tests/test_abi_cpu.py compares this table and the mirrors above with the header).
# Pointers to host structs are POINTER(mirror); device pointers, descriptor tables on the device among them, are c_void_p.
_P, _I, _L, _U32, _U64, _F, _LONG, _SZ = C.c_void_p, C.c_int, C.c_int64, C.c_uint32, C.c_uint64, C.c_float, C.c_long, C.c_size_t
_DROP = (_F, _U32, _U64)            # a dropout's (p, site, seed)
SIGNATURES = {
    'a4r_version': (_I, ()),
    'a4r_gemm_nt': (_I, (_P, C.POINTER(GemmArgs))),
    'a4r_gemm_tail_plan': (_I, (_I, _I, _P, _P)),
    'a4r_gemm_tail_max': (_I, (_I,)),
    'a4r_gemm_rows_256': (_I, (_I, _I)),
    'a4r_gemm_variant': (_I, (_I,)),
    'a4r_gemm_tn': (_I, (_P, _P, _I, _P, _I, _P, _I, _I, _I, _I, _I)),
    'a4r_gemm_tn_bias': (_I, (_P, _P, _I, _P, _I, _P, _I, _I, _I, _I, _I, _P)),
    'a4r_gemm_tn_multi': (_I, (_P, C.POINTER(TnProb), _I, _I, _I)),
    'a4r_sasrec_block_fwd': (_I, (_P, C.POINTER(SasrecBlock), _P, _P, _P, _I, _I, _I)),
    'a4r_sasrec_block_bwd': (_I, (_P, C.POINTER(SasrecBlock), _P, _P, _P, _P, _I, _I, _I)),
    'a4r_gemm_tn2': (_I, (_P,) + (_P, _I, _P, _I, _P, _I, _I, _I) * 2 + (_I, _I, _P, _P)),
    'a4r_colsum': (_I, (_P, _P, _I, _P, _I, _I, _I)),
    'a4r_adapter_ln_fwd': (_I, (_P, _P, _I, _P, _I, _P, _I, _P, _P, _P, _P, _P, _P, _F, _I, _P, _P, _P, _I, _P, _I, _P, _I, _I, _I, _I,
                                _P, _I, _P, _P, _I, _P, _I, _I)),
    'a4r_adapter_ln_bwd': (_I, (_P, _P, _I, _P, _I, _P, _P, _P, _I, _P, _I, _P, _P, _I, _P, _I, _P, _P, _I, _P, _P, _P, _I, _I, _I, _I) + _DROP + (_P, _I, _P)),
    'a4r_attn_fwd': (_I, (_P, C.POINTER(AttnArgs))),
    'a4r_attn_bwd': (_I, (_P, C.POINTER(AttnArgs))),
    'a4r_attn_long_fwd': (_I, (_P, C.POINTER(AttnArgs), _P)),
    'a4r_attn_long_bwd': (_I, (_P, C.POINTER(AttnArgs), _P, _P)),
    'a4r_patchify': (_I, (_P, _P, _I, _P, _I, _P, _I, _I, _I, _I, _I, _I, _I)),
    'a4r_vit_assemble': (_I, (_P, _P, _I, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I)),
    'a4r_mae_keep_indices': (_I, (_P, _P, _P, _I, _I, _I, _U64, _U32)),
    'a4r_resample_u8': (_I, (_P, _P, _P, _P, _P, _I, _LONG, _I, _I, _LONG)),
    'a4r_embed_ln': (_I, (_P, _P, _I, _P, _P, _P, _P, _P, _F, _P, _I, _I, _I, _I, _I, _I, _I) + _DROP + (_P, _P, _P)),
    'a4r_embed_bwd': (_I, (_P, _P, _I, _P, _I, _P, _P, _I, _I, _I, _I, _I, _I)),
    'a4r_ln_fwd': (_I, (_P, _P, _I, _P, _I, _P, _P, _F, _P, _I, _P, _I, _I, _I) + _DROP),
    'a4r_ln_fwd_sum': (_I, (_P, _P, _I, _P, _I, _P, _I, _P, _P, _F, _P, _I, _P, _I, _P, _I, _P, _I, _P, _I, _I, _I)),
    'a4r_ln_fwd_fp8': (_I, (_P, _P, _I, _P, _I, _P, _P, _F, _P, _I, _P, _I, _P, _P, _I, _I, _I)),
    'a4r_quant_rows_fp8': (_I, (_P, _P, _I, _P, _I, _P, _I, _I, _I)),
    'a4r_ln_bwd': (_I, (_P, _P, _I, _P, _I, _P, _I, _P, _P, _P, _I, _P, _I, _P, _P, _P, _I, _I, _I) + _DROP + (_P, _I) + _DROP),
    'a4r_gather_rows': (_I, (_P, _P, _I, _P, _I, _I, _I, _I, _I)),
    'a4r_scatter_rows': (_I, (_P, _P, _I, _P, _I, _I, _I, _I, _I)),
    'a4r_rows_idx_copy': (_I, (_P, _P, _L, _P, _L, _P, _I, _L, _I)),
    'a4r_scatter_rows_fill': (_I, (_P, _P, _I, _P, _I, _I, _I, _I, _I, _I)),
    'a4r_dropout_apply': (_I, (_P, _P, _I, _P, _I, _I, _I, _I) + _DROP),
    'a4r_act_bwd_f32': (_I, (_P, _P, _P, _P, _L, _I)),
    'a4r_score_bce_fwd': (_I, (_P,) * 7 + (_I,) * 4),
    'a4r_score_bce_bwd': (_I, (_P,) * 7 + (_F, _P, _P, _P) + (_I,) * 4),
    'a4r_emb_grad_add_inputs': (_I, (_P, _P, _I, _P, _I, _I, _I)),
    'a4r_take_inputs': (_I, (_P, _P, _P, _I, _I, _I, _I)),
    'a4r_adam_step': (_I, (_P, _P, _P, _P, _P, _L, _P, _P, _I, _P, _I, _F, _F, _F, _F)),
    'a4r_grad_sumsq': (_I, (_P, _P, _L, _F, _P)),
    'a4r_adamw_step': (_I, (_P, _P, _P, _P, _P, _L, _P, _P, _I, _P, _I, _F, _F, _F, _F, _P, _I, _P, _F, _P)),
    'a4r_pack_matrices': (_I, (_P, _P, _P, _I, _I, _I)),
    'a4r_lora_merge': (_I, (_P, _P, _P, _P, _F, _P, _I, _P, _I, _I, _I, _I, _I)),
    'a4r_lora_merge_batch': (_I, (_P, _P, _I, _I, _I)),
    'a4r_lora_bwd_fused': (_I, (_P, _P, _I, _P, _P, _I, _P, _P, _P, _P, _I, _F, _F, _P, _P, _I, _P, _P, _I, _P, _P, _I, _I, _I, _I, _I, _P, _L)),
    'a4r_lora_bwd_fused_ws_floats': (_I, (_I,)),
    'a4r_phm_build': (_I, (_P, _P, _P, _I, _P)),
    'a4r_phm_bwd': (_I, (_P, _P, _P, _I, _P)),
    'a4r_unpack_add': (_I, (_P, _P, _P, _I, _I)),
    'a4r_memset_zero': (_I, (_P, _P, _L)),
    'a4r_eval_rank': (_I, (_P,) * 7 + (_I,) * 3),
    'a4r_topk_ws_bytes': (_SZ, (_I, _I, _I)),
    'a4r_topk_items': (_I, (_P,) * 8 + (_I,) * 4),
    'a4r_score_ce_ws_bytes': (_SZ, (_I, _I, _I, _I)),
    'a4r_score_ce_ranges': (_I, (_I, _I)),
    'a4r_score_ce_fwd': (_I, (_P,) * 9 + (_I,) * 4),
    'a4r_score_ce_bwd_rows': (_I, (_P,) * 7 + (_F, _P, _P, _P) + (_I,) * 4),
    'a4r_score_ce_bwd_items': (_I, (_P,) * 7 + (_F, _P, _P) + (_I,) * 4),
    'a4r_id_index': (_I, (_P, _P, _I, _I) + (_P,) * 7 + (_L,)),
    'a4r_id_index_ws_ints': (_I, (_I, _I)),
    'a4r_id_grad_sum': (_I, (_P, _P, _I, _P, _P, _P, _P, _I, _P, _I, _I)),
    'a4r_id_sample': (_I, (_P, _P, _I, _I, _P, _I, _I, _U64, _U64, _I, _P, _P, _P)),
    'a4r_encoder_layer_fwd': (_I, (_P, C.POINTER(EncoderLayer), _P, _P, _P)),
    'a4r_encoder_layer_bwd': (_I, (_P, C.POINTER(EncoderLayer), _P, _P, _P, _P)),
}
EXPORTS = list(SIGNATURES)


_lib = None


def lib():
    """Load the HIP library once; fail loudly when it is absent."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f'{LIB_PATH} not found: build it with `python -c "import __graft_entry__ as g; g.build()"` '
                '(hipcc --offload-arch=gfx950).  adapter4rec_amd has no CPU / PyTorch fallback.')
        _lib = C.CDLL(LIB_PATH)
        tables = dict(SIGNATURES)
        for module, (table, _) in SATELLITES.items():                # (the satellites' exports: a table each, bottom of this file)
            tables.update(getattr(importlib.import_module('.' + module, __package__), table))
        missing = [name for name in tables if not hasattr(_lib, name)]
        if missing:                   # a build from before an entry point was added (additions keep the ABI number: no argument list changes)
            _lib = None
            raise RuntimeError(f'{LIB_PATH} lacks {", ".join(missing)}: rebuild it (make -C adapter4rec_amd/csrc)')
        for name, (restype, argtypes) in tables.items():
            f = getattr(_lib, name)
            f.restype, f.argtypes = restype, argtypes
        got = _lib.a4r_version()
        if got != ABI_VERSION:        # an older A/B build has every export but other argument lists: calling it would pass shifted pointers
            _lib = None
            raise RuntimeError(f'{LIB_PATH} has ABI version {got}, this binding is for {ABI_VERSION}: rebuild it (make -C adapter4rec_amd/csrc)')
    return _lib


def _check(rc, what):
    if rc != 0:
        raise RuntimeError(f'{what} failed with status {rc} ' + {-1: '(invalid argument)', -2: '(launch failure)'}.get(rc, ''))


_DEV_INDEX = None


def _stream():
    """torch's CURRENT stream on this process's device as a raw hipStream_t.  One process drives one GPU, so the device index is
    resolved once; torch._C._cuda_getCurrentRawStream is the accessor torch's own extensions use (torch.cuda.current_stream()
    builds a Stream object per call: 8 us x 400 launches per step)."""
    global _DEV_INDEX
    if _DEV_INDEX is None:
        _DEV_INDEX = torch.cuda.current_device()
    return torch._C._cuda_getCurrentRawStream(_DEV_INDEX)


def _p(t):
    return t.data_ptr() if t is not None else None


def _dt(t):
    if t.dtype == torch.bfloat16:
        return BF16
    if t.dtype == torch.float32:
        return F32
    if t.dtype == torch.uint8:           # e4m3 bit patterns (a4r_quant_rows_fp8 / a4r_ln_fwd_fp8 / quantize_weight_fp8)
        return FP8
    raise TypeError(f'unsupported dtype {t.dtype}')


def _ld(t):
    assert t.dim() == 2 and t.stride(1) == 1, 'row-major 2-D tensor expected'
    return t.stride(0)


def _ld0(t):
    return _ld(t) if t is not None else 0


def require_gpu(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise RuntimeError('adapter4rec_amd kernels need device tensors (no CPU fallback)')


# ------------------------------------------------------------------ wrappers
def gemm_nt(A, B, Cout, bias=None, C2=None, R1=None, R2=None, Pre=None, act=0, dact=0, alpha=1.0,
            drop_p=0.0, drop_site=0, drop_seed=0, M=None, drop_first=False, c2_deriv=False, scale_a=None, scale_b=None,
            c_fp8=0, c_scale=1.0, c_scale_out=None, q8_tiled=False):
    """q8_tiled: the 8-bit derivative tensor (C2 with c2_deriv='q8' / Pre with DACT_MUL_Q8) in the 256-tile kernel's own order (include/a4r.h).
    c_fp8 (fp8 operands only): Cout is a uint8 tensor that receives the result as e4m3 bytes (include/a4r.h: 1 = static scale c_scale,
    2 = row m scaled by scale_a[m] * c_scale, that product written to c_scale_out[m])."""
    if not (A.is_cuda and B.is_cuda and Cout.is_cuda):
        require_gpu(A, B, Cout)
    N, K = B.shape
    din, dout = _dt(A), _dt(Cout)
    if c_fp8:
        assert din == FP8 and Cout.dtype == torch.uint8 and R1 is None and R2 is None and (c_fp8 == 1 or c_scale_out is not None)
        dout = BF16
    assert A.shape[1] == K and Cout.shape[1] == N and _dt(B) == din
    q8c, q8p = c2_deriv == 'q8', dact == DACT_MUL_Q8
    for t, q8 in ((C2, q8c), (R1, False), (R2, False), (Pre, q8p)):
        assert t is None or (t.dtype == torch.uint8 if q8 else _dt(t) == dout)
    assert bias is None or bias.dtype == torch.float32
    # positional construction (field order of a4r_gemm_t): one C call instead of ~30 attribute stores -- this wrapper runs
    # ~220 times per training step
    g = GemmArgs(A.data_ptr(), B.data_ptr(), Cout.data_ptr(), _p(bias), _p(C2), _p(R1), _p(R2), _p(Pre),
                 A.shape[0] if M is None else M, N, K, _ld(A), _ld(B), _ld(Cout),
                 _ld(C2) if C2 is not None else 0, _ld(R1) if R1 is not None else 0, _ld(R2) if R2 is not None else 0,
                 _ld(Pre) if Pre is not None else 0, din, dout, act, dact, int(drop_first), 2 if q8c else int(bool(c2_deriv)), alpha, drop_p, drop_site,
                 drop_seed, 0, _p(scale_a), _p(scale_b), int(c_fp8), float(c_scale), _p(c_scale_out), int(bool(q8_tiled)))
    _check(lib().a4r_gemm_nt(_stream(), C.byref(g)), 'a4r_gemm_nt')


def gemm_variant(v):
    return lib().a4r_gemm_variant(v)


def gemm_tail_max(k):
    return lib().a4r_gemm_tail_max(k)


def gemm_tail_plan(M, N):
    """(p_full, kp): row panels of full 256-row tiles and the height / 32 of the short tiles behind them (kp = 0: none)."""
    pf, kp = C.c_int(0), C.c_int(0)
    lib().a4r_gemm_tail_plan(M, N, C.byref(pf), C.byref(kp))
    return pf.value, kp.value


def gemm_rows_256(M, N):
    """Leading rows of an [M, N] gemm_nt output that the 256-tile kernel computes (= the tile-native part of a q8_tiled tensor)."""
    return lib().a4r_gemm_rows_256(M, N)


def adapter_ln_ok(A, d):
    """Shapes the one-launch adapter kernels (a4r_adapter_ln_fwd / _bwd) are instantiated for."""
    return A.dtype == torch.bfloat16 and d == 64 and A.shape[1] in (128, 256, 512, 768, 1024)


def adapter_ln_fwd(A, R1, R2, Wd, bd, Wu, bu, gamma, beta, eps, act, zp, z, v, y, stats, M=None, y8=None, ys=None, res32=None, y32=None, frag=None):
    """res32 / y32 (fp32 [M, H], optional): the residual operand that is not A read in fp32, and y before its bf16 rounding (include/a4r.h).
    The same two as int8 [M, H] (--residual_dtype bf24, w_frag bit 1): byte planes beside the bf16 tensors -- residual read / y written as 24-bit floats;
    as int8 [M, H / 2] (--residual_dtype bf20, w_frag bits 1 + 2): nibble planes, 20-bit floats.
    frag = (Wd_f, Wu_f): the same matrices in fragment order (a4r_pack_matrices layouts 1 / 2): read instead of Wd / Wu (w_frag)."""
    require_gpu(A, R1, R2, v, y, res32, y32)
    M = A.shape[0] if M is None else M
    assert y is not None or y8 is not None
    twins = [t for t in (res32, y32) if t is not None]
    lo8 = bool(twins) and twins[0].dtype == torch.int8
    assert all(t.dtype == (torch.int8 if lo8 else torch.float32) and t.shape[0] >= M for t in twins)
    lo4 = lo8 and twins[0].shape[1] == A.shape[1] // 2
    assert not lo8 or all(t.shape[1] == (A.shape[1] // 2 if lo4 else A.shape[1]) for t in twins)
    wd_, wu_ = (Wd, Wu) if frag is None else frag
    _check(lib().a4r_adapter_ln_fwd(_stream(), _p(A), _ld(A), _p(R1), _ld(R1), _p(R2), _ld0(R2), _p(wd_), _p(bd), _p(wu_), _p(bu), _p(gamma), _p(beta), eps, act, _p(zp), _p(z),
                                    _p(v), _ld0(v), _p(y), _ld0(y), _p(stats), M, A.shape[1], Wd.shape[0], _dt(A), _p(y8), _ld0(y8), _p(ys), _p(res32), _ld0(res32), _p(y32),
                                    _ld0(y32), (0 if frag is None else 1) | (2 if lo8 else 0) | (4 if lo4 else 0)), 'a4r_adapter_ln_fwd')


def adapter_ln_bwd(dy, v, stats, gamma, dres, zp, act, WuT, WdT, inner_res, dv, dzp, dh, dgamma=None, dbeta=None, dbias=None, M=None,
                   drop_p=0.0, drop_site=0, drop_seed=0, dbd=None, bias_total=False, beta_y=None, frag=None):
    """beta_y: the forward kept y = LN(v) instead of v (called with v=None); `v` is that y and xhat is rebuilt as (y - beta_y) / gamma.
    frag = (WuT_f, WdT_f): the two matrices in fragment order (flags bit 1)."""
    require_gpu(dy, v, dv, dh)
    M = dy.shape[0] if M is None else M
    wut_, wdt_ = (WuT, WdT) if frag is None else frag
    _check(lib().a4r_adapter_ln_bwd(_stream(), _p(dy), _ld(dy), _p(v), _ld(v), _p(stats), _p(gamma), _p(dres), _ld0(dres), _p(zp), act, _p(wut_), _p(wdt_), int(inner_res), _p(dv),
                                    _ld(dv), _p(dzp), _p(dh), _ld(dh), _p(dgamma), _p(dbeta), _p(dbias), M, dy.shape[1], WuT.shape[0], _dt(dy), drop_p, drop_site, drop_seed,
                                    _p(dbd), int(bias_total) | (0 if frag is None else 2), _p(beta_y)), 'a4r_adapter_ln_bwd')


def sasrec_block(desc, x, log_mask, out, n_users, T, train, dy=None):
    """a4r_sasrec_block_fwd (dy None: out = y) / a4r_sasrec_block_bwd (out = dx; the adapter gradients are added into desc.g_*).
    desc: dict of the a4r_sasrec_block_t fields (tensors for the pointer fields, None = null)."""
    require_gpu(x, log_mask, out, dy)
    assert x.dtype == torch.float32 and out.dtype == torch.float32 and log_mask.dtype == torch.float32 and x.shape[1] == 64 and x.is_contiguous() and out.is_contiguous()
    b = SasrecBlock()
    for k, v in desc.items():
        setattr(b, k, (v.data_ptr() if v is not None else None) if (k in SasrecBlock._PTRS or k in ('ln3_g', 'ln3_b', 'g_ln3_g', 'g_ln3_b')) else v)
    if dy is None:
        _check(lib().a4r_sasrec_block_fwd(_stream(), C.byref(b), _p(x), _p(log_mask), _p(out), n_users, T, int(train)), 'a4r_sasrec_block_fwd')
    else:
        assert dy.dtype == torch.float32 and dy.is_contiguous()
        _check(lib().a4r_sasrec_block_bwd(_stream(), C.byref(b), _p(x), _p(log_mask), _p(dy), _p(out), n_users, T, int(train)), 'a4r_sasrec_block_bwd')


def gemm_tn(X, Y, Cacc, M=None):
    require_gpu(X, Y, Cacc)
    assert Cacc.dtype == torch.float32 and _dt(X) == _dt(Y)
    M = X.shape[0] if M is None else M
    _check(lib().a4r_gemm_tn(_stream(), _p(X), _ld(X), _p(Y), _ld(Y), _p(Cacc), _ld(Cacc), M, X.shape[1], Y.shape[1], _dt(X)), 'a4r_gemm_tn')


def gemm_tn_bias(X, Y, Cacc, xsum, M=None):
    """Cacc += X^T Y and xsum[:P] += column sums of X (a trainable Linear's dW and db from one pass over dy)."""
    require_gpu(X, Y, Cacc, xsum)
    assert Cacc.dtype == torch.float32 and xsum.dtype == torch.float32 and xsum.numel() >= X.shape[1] and _dt(X) == _dt(Y)
    M = X.shape[0] if M is None else M
    _check(lib().a4r_gemm_tn_bias(_stream(), _p(X), _ld(X), _p(Y), _ld(Y), _p(Cacc), _ld(Cacc), M, X.shape[1], Y.shape[1], _dt(X), _p(xsum)), 'a4r_gemm_tn_bias')


def gemm_tn_multi(probs, M=None):
    """probs: 1..4 tuples (X, Y, Cacc, xsum or None) over the same M rows: Cacc += X^T Y, xsum += column sums of X (include/a4r.h: a4r_gemm_tn_multi)."""
    assert 1 <= len(probs) <= 4
    arr = (TnProb * len(probs))()
    dt = _dt(probs[0][0])
    M = probs[0][0].shape[0] if M is None else M
    for a, (X, Y, Cacc, xsum) in zip(arr, probs):
        require_gpu(X, Y, Cacc, xsum)
        assert Cacc.dtype == torch.float32 and _dt(X) == dt and _dt(Y) == dt and (xsum is None or (xsum.dtype == torch.float32 and xsum.numel() >= X.shape[1]))
        a.X, a.Y, a.C, a.xsum = X.data_ptr(), Y.data_ptr(), Cacc.data_ptr(), (xsum.data_ptr() if xsum is not None else None)
        a.ldx, a.ldy, a.ldc, a.P, a.Q = _ld(X), _ld(Y), _ld(Cacc), X.shape[1], Y.shape[1]
    _check(lib().a4r_gemm_tn_multi(_stream(), arr, len(probs), M, dt), 'a4r_gemm_tn_multi')


def gemm_tn2(X1, Y1, C1, X2, Y2, C2, M=None, xsum1=None, xsum2=None):
    """C1 += X1^T Y1 and C2 += X2^T Y2 over the same M rows, one launch (bf16; equal tile counts); xsum_k[p] += column sums of X_k."""
    require_gpu(X1, Y1, C1, X2, Y2, C2, xsum1, xsum2)
    assert C1.dtype == torch.float32 and C2.dtype == torch.float32
    assert (xsum1 is None or (xsum1.dtype == torch.float32 and xsum1.numel() >= X1.shape[1])) and (xsum2 is None or (xsum2.dtype == torch.float32 and xsum2.numel() >= X2.shape[1]))
    M = X1.shape[0] if M is None else M
    _check(lib().a4r_gemm_tn2(_stream(), _p(X1), _ld(X1), _p(Y1), _ld(Y1), _p(C1), _ld(C1), X1.shape[1], Y1.shape[1], _p(X2), _ld(X2), _p(Y2), _ld(Y2), _p(C2), _ld(C2),
                              X2.shape[1], Y2.shape[1], M, _dt(X1), _p(xsum1), _p(xsum2)), 'a4r_gemm_tn2')


def colsum(X, out, M=None):
    require_gpu(X, out)
    M = X.shape[0] if M is None else M
    _check(lib().a4r_colsum(_stream(), _p(X), _ld(X), _p(out), M, X.shape[1], _dt(X)), 'a4r_colsum')


def _attn_args(qkv, q_off, k_off, v_off, key_mask, n_items, S, n_heads, dh, causal, scale, mask_neg, drop_p, drop_site, drop_seed, offsets=None):
    a = AttnArgs()
    if offsets is not None:
        require_gpu(offsets)
        assert offsets.dtype == torch.int32 and offsets.numel() >= n_items + 1
    a.offsets = _p(offsets)
    a.qkv, a.ld, a.q_off, a.k_off, a.v_off = _p(qkv), _ld(qkv), q_off, k_off, v_off
    a.key_mask = _p(key_mask)
    a.n_items, a.S, a.n_heads, a.dh, a.causal, a.dtype = n_items, S, n_heads, dh, int(causal), _dt(qkv)
    a.scale, a.mask_neg = scale, mask_neg
    a.drop_p, a.drop_site, a.drop_seed = drop_p, drop_site, drop_seed
    return a


def attn_fwd(qkv, out, key_mask, n_items, S, n_heads, dh, q_off, k_off, v_off, causal, scale, mask_neg,
             drop_p=0.0, drop_site=0, drop_seed=0, offsets=None):
    """offsets (int32 [n_items + 1] on the device): packed items, see a4r_attn_t.offsets"""
    require_gpu(qkv, out)
    a = _attn_args(qkv, q_off, k_off, v_off, key_mask, n_items, S, n_heads, dh, causal, scale, mask_neg, drop_p, drop_site, drop_seed, offsets)
    a.out, a.ldo = _p(out), _ld(out)
    _check(lib().a4r_attn_fwd(_stream(), C.byref(a)), 'a4r_attn_fwd')


def attn_bwd(qkv, dout, dqkv, key_mask, n_items, S, n_heads, dh, q_off, k_off, v_off, causal, scale, mask_neg,
             drop_p=0.0, drop_site=0, drop_seed=0, offsets=None):
    require_gpu(qkv, dout, dqkv)
    assert _ld(dqkv) == _ld(qkv)
    a = _attn_args(qkv, q_off, k_off, v_off, key_mask, n_items, S, n_heads, dh, causal, scale, mask_neg, drop_p, drop_site, drop_seed, offsets)
    a.dout, a.ldo, a.dqkv = _p(dout), _ld(dout), _p(dqkv)
    _check(lib().a4r_attn_bwd(_stream(), C.byref(a)), 'a4r_attn_bwd')


def attn_long_fwd(qkv, out, lse, n_items, S, n_heads, dh, q_off, k_off, v_off, scale, drop_p=0.0, drop_site=0, drop_seed=0, key_mask=None, causal=False):
    """key_mask (fp32 [n_items, S], 1 = attend; optional, head width 64): HF's attention_mask -- text towers with more than 32 tokens per title"""
    require_gpu(qkv, out, lse, key_mask)
    assert lse.dtype == torch.float32 and lse.numel() >= n_items * n_heads * S
    a = _attn_args(qkv, q_off, k_off, v_off, key_mask, n_items, S, n_heads, dh, causal, scale, 0.0, drop_p, drop_site, drop_seed)
    a.out, a.ldo = _p(out), _ld(out)
    _check(lib().a4r_attn_long_fwd(_stream(), C.byref(a), _p(lse)), 'a4r_attn_long_fwd')


def attn_long_bwd(qkv, out, dout, dqkv, lse, delta_ws, n_items, S, n_heads, dh, q_off, k_off, v_off, scale,
                  drop_p=0.0, drop_site=0, drop_seed=0, key_mask=None, causal=False):
    """out: the ctx attn_long_fwd wrote (backward takes delta = dO . O from it)."""
    require_gpu(qkv, out, dout, dqkv, lse, delta_ws, key_mask)
    assert _ld(dqkv) == _ld(qkv) and delta_ws.dtype == torch.float32 and delta_ws.numel() >= n_items * n_heads * S
    a = _attn_args(qkv, q_off, k_off, v_off, key_mask, n_items, S, n_heads, dh, causal, scale, 0.0, drop_p, drop_site, drop_seed)
    assert _ld(out) == _ld(dout)
    a.out, a.dout, a.ldo, a.dqkv = _p(out), _p(dout), _ld(dout), _p(dqkv)
    _check(lib().a4r_attn_long_bwd(_stream(), C.byref(a), _p(lse), _p(delta_ws)), 'a4r_attn_long_bwd')


def encoder_layer_fwd(desc, x, x1, x_out):
    """a4r_encoder_layer_fwd: the 7 launches of one post-LN encoder layer with serial Houlsby adapters from ONE call (desc: EncoderLayer)."""
    require_gpu(x, x1, x_out)
    _check(lib().a4r_encoder_layer_fwd(_stream(), C.byref(desc), _p(x), _p(x1), _p(x_out)), 'a4r_encoder_layer_fwd')


def encoder_layer_bwd(desc, x1, x_out, dx_out, dx_in):
    """a4r_encoder_layer_bwd: its 9 backward launches (dx_in None: the d qkv product is skipped)."""
    require_gpu(x1, x_out, dx_out, dx_in)
    _check(lib().a4r_encoder_layer_bwd(_stream(), C.byref(desc), _p(x1), _p(x_out), _p(dx_out), _p(dx_in)), 'a4r_encoder_layer_bwd')


def patchify(img, out, patch, keep_idx=None):
    """img fp32 [n, C, H, W] (normalised) or uint8 [n, H, W, C] (raw) -> out [n * n_keep, >= C*patch*patch]."""
    require_gpu(img, out)
    assert img.is_contiguous()
    if img.dtype == torch.uint8:
        kind, (n, Hi, Wi, Cc) = 1, img.shape
    else:
        assert img.dtype == torch.float32
        kind, (n, Cc, Hi, Wi) = 0, img.shape
    n_keep = keep_idx.shape[1] if keep_idx is not None else (Hi // patch) * (Wi // patch)
    assert keep_idx is None or (keep_idx.dtype == torch.int32 and keep_idx.is_contiguous() and keep_idx.shape[0] == n)
    _check(lib().a4r_patchify(_stream(), _p(img), kind, _p(out), _ld(out), _p(keep_idx), n_keep, n, Cc, Hi, Wi, patch, _dt(out)), 'a4r_patchify')


def mae_keep_indices(keep, n_patches, noise=None, seed=0, site=0):
    """keep int32 [n_items, n_keep] <- argsort(noise, 1)[:, :n_keep] (stable); noise None: counter-hash uniform noise drawn on the device."""
    require_gpu(keep, noise)
    assert keep.dtype == torch.int32 and keep.is_contiguous()
    assert noise is None or (noise.dtype == torch.float32 and noise.is_contiguous() and tuple(noise.shape) == (keep.shape[0], n_patches))
    _check(lib().a4r_mae_keep_indices(_stream(), _p(noise), _p(keep), keep.shape[0], n_patches, keep.shape[1], int(seed) & (2 ** 64 - 1), site), 'a4r_mae_keep_indices')


def resample_u8(src, dst, bounds, kk, n_outer, in_len, out_len, inner):
    require_gpu(src, dst, bounds, kk)
    assert src.dtype == torch.uint8 and dst.dtype == torch.uint8 and bounds.dtype == torch.int32 and kk.dtype == torch.int32
    assert src.is_contiguous() and dst.is_contiguous() and src.numel() == n_outer * in_len * inner and dst.numel() == n_outer * out_len * inner
    _check(lib().a4r_resample_u8(_stream(), _p(src), _p(dst), _p(bounds), _p(kk), kk.shape[1], n_outer, in_len, out_len, inner), 'a4r_resample_u8')


def vit_assemble(patches, cls, pos, out, n_items, n_keep, keep_idx=None, tokens_out=0):
    require_gpu(patches, out)
    _check(lib().a4r_vit_assemble(_stream(), _p(patches), _ld(patches), _p(cls), _p(pos), _p(keep_idx), _p(out), _ld(out), n_items, n_keep, cls.numel(), _dt(out), tokens_out),
           'a4r_vit_assemble')


def embed_bwd(ids, dpre, dword, dpos, n_items, S, roberta=False, pad_id=0):
    """dword[id] += dpre[row], dpos[pos_id] += dpre[row] over the n_items * S token rows (include/a4r.h), padding rows skipped.  The kernel
    indexes the tables with H = dpre.shape[1] and does not bound the ids: the shapes are checked here, before any launch.  The vocabulary
    bound (ids < dword.shape[0]) is the caller's: checking it would read the ids back from the device."""
    H = dpre.shape[1]
    assert ids.dtype == torch.int64 and ids.dim() == 2 and ids.stride(1) == 1, 'ids: int64 [n_items, >= S] with unit column stride'
    assert ids.shape[0] >= n_items and ids.shape[1] >= S, f'ids {tuple(ids.shape)} smaller than [{n_items}, {S}]'
    assert dpre.dim() == 2 and dpre.shape[0] >= n_items * S, f'dpre {tuple(dpre.shape)}: fewer than {n_items * S} rows'
    for name, t in (('dword', dword), ('dpos', dpos)):
        assert t is None or (t.dtype == torch.float32 and t.dim() == 2 and t.is_contiguous() and t.shape[1] == H), \
            f'{name}: contiguous fp32 [rows, {H}] expected, got {None if t is None else (t.dtype, tuple(t.shape), t.stride())}'
    n_pos = S + pad_id + 1 if roberta else S         # largest pos_id + 1 (RoBERTa: cumsum(id != pad) + pad <= S + pad)
    assert dpos is None or dpos.shape[0] >= n_pos, f'dpos has {dpos.shape[0]} rows, position ids reach {n_pos - 1}'
    require_gpu(ids, dpre, dword, dpos)
    _check(lib().a4r_embed_bwd(_stream(), _p(ids), ids.stride(0), _p(dpre), _ld(dpre), _p(dword), _p(dpos), n_items, S, dpre.shape[1], int(roberta), pad_id, _dt(dpre)),
           'a4r_embed_bwd')


def embed_ln(ids, word, pos, type0, gamma, beta, eps, out, n_items, S, roberta=False, pad_id=0,
             drop_p=0.0, drop_site=0, drop_seed=0, pre_out=None, stats_out=None, key_mask_out=None):
    require_gpu(ids, word, out)
    assert ids.dtype == torch.int64 and ids.stride(1) == 1
    _check(lib().a4r_embed_ln(_stream(), _p(ids), ids.stride(0), _p(word), _p(pos), _p(type0), _p(gamma), _p(beta), eps, _p(out), _ld(out), n_items, S, word.shape[1], int(roberta),
                              pad_id, _dt(out), drop_p, drop_site, drop_seed, _p(pre_out), _p(stats_out), _p(key_mask_out)), 'a4r_embed_ln')


def quantize_weight_fp8(w):
    """Frozen weight [out, in] -> (e4m3 bit patterns uint8 [out, in], fp32 scale [out]): per-output-channel absmax scaling, the B
    operand form of the fp8 a4r_gemm_nt.  Build-time only (once per frozen matrix)."""
    wf = w.detach().float()
    amax = wf.abs().amax(1).clamp_min(1e-30)
    q = (wf * (448.0 / amax)[:, None]).to(torch.float8_e4m3fn).view(torch.uint8).contiguous()
    return q, (amax / 448.0).contiguous()


def quant_rows_fp8(x, q, scale, M=None):
    require_gpu(x, q, scale)
    M = x.shape[0] if M is None else M
    assert q.dtype == torch.uint8 and scale.dtype == torch.float32
    _check(lib().a4r_quant_rows_fp8(_stream(), _p(x), _ld(x), _p(q), _ld(q), _p(scale), M, x.shape[1], _dt(x)), 'a4r_quant_rows_fp8')


def _ln_operands(M, H, gamma, beta=None, stats=None, add=None):
    """What the LayerNorm kernels read through a bare pointer: gamma / beta as H contiguous fp32, add as contiguous [add_rows, H] fp32 (its leading
    dimension IS H), stats as contiguous [>= M, 2] fp32.  A strided view would be misread silently."""
    f32 = torch.float32
    assert gamma.dtype is f32 and gamma.is_contiguous() and gamma.numel() >= H, f'gamma: {H} contiguous fp32 values expected'
    assert beta is None or (beta.dtype is f32 and beta.is_contiguous() and beta.numel() >= H), f'beta: {H} contiguous fp32 values expected'
    assert add is None or (add.dtype is f32 and add.dim() == 2 and add.shape[1] == H and add.shape[0] > 0 and add.is_contiguous()), \
        'add: a contiguous fp32 [add_rows, H] table expected'
    assert stats is None or (stats.dtype is f32 and stats.dim() == 2 and stats.shape[1] == 2 and stats.shape[0] >= M and stats.is_contiguous()), \
        'stats: contiguous fp32 [>= M, 2] expected'


def ln_fwd_sum(h, res, gamma, beta, eps, y, stats, M=None, res32=None, sum_out=None, sum32=None, y32=None):
    """y = LN(h + residual), sum in fp32, normalised unrounded; residual = res32 (fp32) when given, else res (h's dtype).  Optional outputs:
    sum_out (h's dtype), sum32, y32 (fp32)."""
    require_gpu(h, res, res32, y, sum_out, sum32, y32)
    M = h.shape[0] if M is None else M
    assert res32 is not None or res is not None
    _ln_operands(M, h.shape[1], gamma, beta, stats)
    _check(lib().a4r_ln_fwd_sum(_stream(), _p(h), _ld(h), _p(res32), _ld0(res32), _p(res), _ld0(res), _p(gamma), _p(beta), eps, _p(y), _ld(y), _p(sum_out), _ld0(sum_out),
                                _p(sum32), _ld0(sum32), _p(y32), _ld0(y32), _p(stats), M, h.shape[1], _dt(h)), 'a4r_ln_fwd_sum')


def ln_fwd(v, gamma, beta, eps, y, stats, M=None, add=None, drop_p=0.0, drop_site=0, drop_seed=0, y8=None, ys=None):
    require_gpu(v, y, y8)
    M = v.shape[0] if M is None else M
    _ln_operands(M, v.shape[1], gamma, beta, stats, add)
    if y8 is not None:                    # also emit the row as e4m3 + per-row scale (y may be None)
        assert drop_p == 0.0 and y8.dtype == torch.uint8 and ys.dtype == torch.float32
        _check(lib().a4r_ln_fwd_fp8(_stream(), _p(v), _ld(v), _p(add), add.shape[0] if add is not None else 0, _p(gamma), _p(beta), eps, _p(y), _ld0(y), _p(y8), _ld(y8), _p(ys),
                                    _p(stats), M, v.shape[1], _dt(v)), 'a4r_ln_fwd_fp8')
        return
    _check(lib().a4r_ln_fwd(_stream(), _p(v), _ld(v), _p(add), add.shape[0] if add is not None else 0, _p(gamma), _p(beta), eps, _p(y), _ld(y), _p(stats), M, v.shape[1], _dt(v),
                            drop_p, drop_site, drop_seed), 'a4r_ln_fwd')


def ln_bwd(dy, v, stats, gamma, dv, M=None, add=None, dgamma=None, dbeta=None, dbias=None, dres=None,
           drop_p=0.0, drop_site=0, drop_seed=0, dv2=None, drop2_p=0.0, drop2_site=0, drop2_seed=0):
    require_gpu(dy, v, dv)
    M = v.shape[0] if M is None else M
    _ln_operands(M, v.shape[1], gamma, None, stats, add)
    _check(lib().a4r_ln_bwd(_stream(), _p(dy), _ld(dy), _p(v), _ld(v), _p(add), add.shape[0] if add is not None else 0, _p(stats), _p(gamma), _p(dres), _ld0(dres), _p(dv), _ld(dv),
                            _p(dgamma), _p(dbeta), _p(dbias), M, v.shape[1], _dt(v), drop_p, drop_site, drop_seed, _p(dv2), _ld0(dv2), drop2_p, drop2_site, drop2_seed),
           'a4r_ln_bwd')


def gather_rows(src, dst, n, row_step):
    require_gpu(src, dst)
    _check(lib().a4r_gather_rows(_stream(), _p(src), _ld(src), _p(dst), _ld(dst), n, row_step, src.shape[1], _dt(src)), 'a4r_gather_rows')


def rows_idx_copy(src, dst, idx, n, scatter=False):
    """dst[r] = src[idx[r]] (scatter: dst[idx[r]] = src[r]) for r < n; 2-D tensors of one dtype, row bytes a multiple of 16; idx int32 on the device."""
    require_gpu(src, dst, idx)
    assert src.dim() == 2 and dst.dim() == 2 and src.dtype == dst.dtype and src.shape[1] == dst.shape[1] and idx.dtype == torch.int32 and idx.numel() >= n
    es = src.element_size()
    _check(lib().a4r_rows_idx_copy(_stream(), _p(src), src.stride(0) * es, _p(dst), dst.stride(0) * es, _p(idx), n, src.shape[1] * es, int(scatter)), 'a4r_rows_idx_copy')


def id_index_ws_ints(n, item_num):
    """int32 elements of a4r_id_index's workspace (a host-side query, no GPU)."""
    k = int(lib().a4r_id_index_ws_ints(n, item_num))
    if k < 0:
        raise RuntimeError(f'a4r_id_index: n = {n}, item_num = {item_num} outside the supported range (include/a4r.h)')
    return k


def id_index(ids, item_num, rows, slots, ptr, uniq, n_uniq, err, ws):
    """a4r_id_index over the n = ids.numel() slot ids (int64, device): rows [n], slots [n], ptr [n + 1], uniq [n], n_uniq [1], err [1] int32 outputs."""
    require_gpu(ids, rows, slots, ptr, uniq, n_uniq, err, ws)
    n = ids.numel()
    assert ids.dtype == torch.int64 and ids.is_contiguous() and ws.dtype == torch.int32
    assert all(t.dtype == torch.int32 for t in (rows, slots, ptr, uniq, n_uniq, err))
    assert rows.numel() >= n and slots.numel() >= n and ptr.numel() >= n + 1 and uniq.numel() >= n
    _check(lib().a4r_id_index(_stream(), _p(ids), n, item_num, _p(rows), _p(slots), _p(ptr), _p(uniq), _p(n_uniq), _p(err), _p(ws), ws.numel()), 'a4r_id_index')


def id_grad_sum(src, slots, ptr, uniq, n_uniq, n, grad):
    """grad[uniq[u]] += the ordered chunked sum of src[slots[ptr[u] .. ptr[u + 1])] for u < *n_uniq (a4r_id_grad_sum); src, grad fp32 2-D."""
    require_gpu(src, slots, ptr, uniq, n_uniq, grad)
    assert src.dtype == torch.float32 and grad.dtype == torch.float32 and src.shape[1] == grad.shape[1] and src.shape[0] >= n
    _check(lib().a4r_id_grad_sum(_stream(), _p(src), _ld(src), _p(slots), _p(ptr), _p(uniq), _p(n_uniq), n, _p(grad), _ld(grad), grad.shape[1]), 'a4r_id_grad_sum')


def scatter_rows(src, dst, n, row_step):
    require_gpu(src, dst)
    _check(lib().a4r_scatter_rows(_stream(), _p(src), _ld(src), _p(dst), _ld(dst), n, row_step, src.shape[1], _dt(src)), 'a4r_scatter_rows')


def scatter_rows_fill(src, dst, n, row_step, fill_rows):
    """dst[r] = src[r / row_step] for r % row_step == 0 (r / row_step < n), 0 elsewhere, r < fill_rows."""
    require_gpu(src, dst)
    _check(lib().a4r_scatter_rows_fill(_stream(), _p(src), _ld(src), _p(dst), _ld(dst), n, row_step, src.shape[1], _dt(src), fill_rows), 'a4r_scatter_rows_fill')


def zero(t):
    """hipMemsetAsync of a contiguous tensor on the current stream."""
    require_gpu(t)
    assert t.is_contiguous()
    _check(lib().a4r_memset_zero(_stream(), _p(t), t.numel() * t.element_size()), 'a4r_memset_zero')


def lora_merge(W, A, B, scaling, dst, dstT, r):
    """dst [out, in] (a row block of the packed qkv operand) and dstT [in, out] (a column block of its transpose) <- W + scaling B A."""
    require_gpu(W, dst, dstT)
    out_f, in_f = W.shape
    assert W.dtype == torch.float32 and W.is_contiguous() and (r == 0 or (A.is_contiguous() and B.is_contiguous()))
    _check(lib().a4r_lora_merge(_stream(), _p(W), _p(A) if r else None, _p(B) if r else None, scaling, _p(dst), _ld(dst), _p(dstT), _ld(dstT), out_f, in_f, r, _dt(dst)),
           'a4r_lora_merge')


def lora_table(entries, device):
    """entries: (W, A, B, scaling, dst, dstT, r) per projection (the arguments of lora_merge) -> (device table, n, max elements, dtype code)."""
    descs = []
    for W, A, B, s, dst, dstT, r in entries:
        assert W.dtype == torch.float32 and W.is_contiguous() and (r == 0 or (A.is_contiguous() and B.is_contiguous())) and _dt(dst) == _dt(entries[0][4])
        descs.append(LoraDesc(W.data_ptr(), A.data_ptr() if r else 0, B.data_ptr() if r else 0, dst.data_ptr(), dstT.data_ptr(), float(s),
                              _ld(dst), _ld(dstT), W.shape[0], W.shape[1], int(r)))
    return desc_table(descs, device), len(descs), max(W.numel() for W, *_ in entries), _dt(entries[0][4])


def lora_merge_batch(tab):
    t, n, mx, code = tab
    _check(lib().a4r_lora_merge_batch(_stream(), _p(t), n, mx, code), 'a4r_lora_merge_batch')


def lora_bwd_fused_ok(x, M, H):
    """the geometry a4r_lora_bwd_fused is built for (everything else keeps the separate products)"""
    return x.dtype == torch.bfloat16 and H == 768 and M % 16 == 0


_lora_ws = {}


def lora_bwd_fused(x, dqa, dqb, Aa, Ab, BTa, BTb, scale_a, scale_b, dAa, dAb, dBa, dBb, dbias_a, dbias_b, M, rank_rows=8):
    """One pass over x, dqa, dqb: dAa | dAb += dt^T x, dBa += dqa^T t_a, dBb += dqb^T t_b (unscaled), dbias_. += column sums (include/a4r.h).  The
    weight operands are views of rank_rows (8, or 16 for ranks 9 - 15) rank rows, the outputs views into the fp32 scratch matrices the corners are
    flushed from."""
    require_gpu(x, dqa, dqb, dAa, dBa)
    H = x.shape[1]
    assert _ld(dqa) == _ld(dqb) and _ld(Aa) == _ld(Ab) == _ld(BTa) == _ld(BTb) and _ld(dAa) == _ld(dAb) and _ld(dBa) == _ld(dBb)
    ldbias = 0
    for bvec in (dbias_a, dbias_b):
        if bvec is not None:
            assert bvec.dtype == torch.float32 and bvec.dim() == 1
            ldbias = bvec.stride(0)
    ws = _lora_ws.get(x.device)                      # the workgroups' column sums before their reduction: one buffer per device (stream-ordered reuse)
    if ws is None:
        ws = _lora_ws[x.device] = torch.empty(int(lib().a4r_lora_bwd_fused_ws_floats(H)), dtype=torch.float32, device=x.device)
    _check(lib().a4r_lora_bwd_fused(_stream(), _p(x), _ld(x), _p(dqa), _p(dqb), _ld(dqa), _p(Aa), _p(Ab), _p(BTa), _p(BTb), _ld(Aa), scale_a, scale_b, _p(dAa), _p(dAb), _ld(dAa),
                                    _p(dBa), _p(dBb), _ld(dBa), _p(dbias_a), _p(dbias_b), ldbias, M, H, _dt(x), rank_rows, _p(ws), ws.numel()), 'a4r_lora_bwd_fused')


def desc_table(entries, device):
    """ctypes descriptor array -> device byte tensor."""
    arr = (type(entries[0]) * len(entries))(*entries)
    return torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(device)


def phm_build(params, desc_dev, n_desc, eff):
    _check(lib().a4r_phm_build(_stream(), _p(params), _p(desc_dev), n_desc, _p(eff)), 'a4r_phm_build')


def phm_bwd(params, desc_dev, n_desc, grads):
    _check(lib().a4r_phm_bwd(_stream(), _p(params), _p(desc_dev), n_desc, _p(grads)), 'a4r_phm_bwd')


def unpack_add(target, desc_dev, n_desc, max_elems):
    _check(lib().a4r_unpack_add(_stream(), _p(target), _p(desc_dev), n_desc, max_elems), 'a4r_unpack_add')


def dropout_apply(x, y, drop_p, drop_site, drop_seed, M=None):
    require_gpu(x, y)
    M = x.shape[0] if M is None else M
    _check(lib().a4r_dropout_apply(_stream(), _p(x), _ld(x), _p(y), _ld(y), M, x.shape[1], _dt(x), drop_p, drop_site, drop_seed), 'a4r_dropout_apply')


def act_bwd_f32(dy, pre, dx, act):
    require_gpu(dy, pre, dx)
    _check(lib().a4r_act_bwd_f32(_stream(), _p(dy), _p(pre), _p(dx), dy.numel(), act), 'a4r_act_bwd_f32')


def score_bce_fwd(emb, prec, log_mask, pos, neg, loss_ws, B, L, E, cpc):
    require_gpu(emb, prec)
    _check(lib().a4r_score_bce_fwd(_stream(), _p(emb), _p(prec), _p(log_mask), _p(pos), _p(neg), _p(loss_ws), B, L, E, int(cpc)), 'a4r_score_bce_fwd')


def score_bce_bwd(emb, prec, log_mask, pos, neg, loss_ws, loss_scale, d_prec, d_emb, B, L, E, cpc, scale_dev=None):
    require_gpu(emb, prec, scale_dev)
    assert scale_dev is None or (scale_dev.dtype == torch.float32 and scale_dev.numel() == 1)
    _check(lib().a4r_score_bce_bwd(_stream(), _p(emb), _p(prec), _p(log_mask), _p(pos), _p(neg), _p(loss_ws), loss_scale, _p(scale_dev), _p(d_prec), _p(d_emb), B, L, E, int(cpc)),
           'a4r_score_bce_bwd')


def score_ce_ranges(R, N1):
    """The library's own item-range count for R rows against an [N1, E] table (a host-side query): <= SCORE_CE_MAX_RANGES and <= the table's
    16-item tiles."""
    k = int(lib().a4r_score_ce_ranges(R, N1))
    if k < 1:
        raise ValueError(f'score_ce_ranges: R = {R} rows and N1 = {N1} table rows (row 0 = the pad item): need R >= 1, N1 >= 2')
    return k


def score_ce_ws_bytes(R, N1, E, ranges=0):
    """Bytes of the workspace a4r_score_ce_fwd / _bwd_rows share (a host-side query); ranges 0 = the library's choice.  0 for arguments the
    kernels refuse.  Independent of N1 at a fixed range count: nothing of size rows x items exists."""
    return int(lib().a4r_score_ce_ws_bytes(R, N1, E, ranges))


def _score_ce_ws(prec, R, N1, E, ranges, ws):
    if ws is None:
        ws = torch.empty(max(score_ce_ws_bytes(R, N1, E, ranges), 16), dtype=torch.uint8, device=prec.device)
    assert ws.is_contiguous() and ws.numel() * ws.element_size() >= score_ce_ws_bytes(R, N1, E, ranges)
    return ws


def _score_ce_check(prec, table, tgt, log_mask, R):
    require_gpu(prec, table, tgt, log_mask)
    assert prec.dim() == 2 and table.dim() == 2 and prec.dtype == torch.float32 and table.dtype == torch.float32
    assert prec.is_contiguous() and table.is_contiguous() and prec.shape[1] == table.shape[1] and prec.shape[0] >= R
    assert tgt.dtype == torch.int32 and tgt.is_contiguous() and tgt.numel() >= R
    assert log_mask.dtype == torch.float32 and log_mask.is_contiguous() and log_mask.numel() >= R


def score_ce_fwd(prec, table, tgt, log_mask, lse, s_tgt, loss_ws, R, ranges=0, ws=None):
    """a4r_score_ce_fwd: full-softmax cross-entropy of the first R rows of prec [>= R, E] against the items 1 .. N1-1 of table [N1, E] (include/a4r.h).
    tgt int32 [R], log_mask fp32 [R]; lse, s_tgt fp32 [R] and loss_ws fp32 [4] (loss, sum, trained rows) are overwritten.  ws: scratch of
    score_ce_ws_bytes bytes (allocated here when None).  The shape arguments go to the library as they are: it answers an unsupported width, R < 1,
    N1 < 2 or ranges outside 0 .. 32 with its invalid-argument status before any launch."""
    _score_ce_check(prec, table, tgt, log_mask, max(R, 0))
    require_gpu(lse, s_tgt, loss_ws)
    assert all(t.dtype == torch.float32 and t.is_contiguous() for t in (lse, s_tgt, loss_ws)) and lse.numel() >= R and s_tgt.numel() >= R and loss_ws.numel() >= 4
    N1, E = table.shape
    ws = _score_ce_ws(prec, R, N1, E, ranges, ws)
    _check(lib().a4r_score_ce_fwd(_stream(), _p(prec), _p(table), _p(tgt), _p(log_mask), _p(lse), _p(s_tgt), _p(loss_ws), _p(ws), R, N1, E, ranges), 'a4r_score_ce_fwd')


def score_ce_bwd(prec, table, tgt, log_mask, lse, loss_ws, loss_scale, d_prec, d_table, R, ranges=0, scale_dev=None, ws=None):
    """The two backward launches of the cross-entropy head (include/a4r.h), both recomputing the scores from prec, table and the forward's lse:
    a4r_score_ce_bwd_rows overwrites d_prec [>= R, E] (contiguous; None: skipped), a4r_score_ce_bwd_items ADDS into d_table [N1, >= E] (row 0
    untouched; None: skipped, a frozen table).  The incoming gradient is loss_scale x scale_dev[0] (scale_dev: a one-element fp32 device tensor)."""
    _score_ce_check(prec, table, tgt, log_mask, max(R, 0))
    require_gpu(lse, loss_ws, d_prec, d_table, scale_dev)
    assert scale_dev is None or (scale_dev.dtype == torch.float32 and scale_dev.numel() == 1)
    N1, E = table.shape
    if d_prec is not None:
        assert d_prec.dtype == torch.float32 and d_prec.is_contiguous() and d_prec.shape[1] == E and d_prec.shape[0] >= R
        ws = _score_ce_ws(prec, R, N1, E, ranges, ws)
        _check(lib().a4r_score_ce_bwd_rows(_stream(), _p(prec), _p(table), _p(tgt), _p(log_mask), _p(lse), _p(loss_ws), loss_scale, _p(scale_dev), _p(d_prec), _p(ws), R, N1, E,
                                           ranges), 'a4r_score_ce_bwd_rows')
    if d_table is not None:
        assert d_table.dtype == torch.float32 and d_table.dim() == 2 and d_table.stride(1) == 1 and d_table.shape[0] >= N1
        _check(lib().a4r_score_ce_bwd_items(_stream(), _p(prec), _p(table), _p(tgt), _p(log_mask), _p(lse), _p(loss_ws), loss_scale, _p(scale_dev), _p(d_table), d_table.stride(0),
                                            R, N1, E), 'a4r_score_ce_bwd_items')


def emb_grad_add_inputs(d_in, d_emb, B, L, E):
    _check(lib().a4r_emb_grad_add_inputs(_stream(), _p(d_in), _ld(d_in), _p(d_emb), B, L, E), 'a4r_emb_grad_add_inputs')


def take_inputs(emb, out, B, L, E):
    _check(lib().a4r_take_inputs(_stream(), _p(emb), _p(out), _ld(out), B, L, E), 'a4r_take_inputs')


def adam_step(p, g, m, v, seg_end, seg_group, group_lr, step, beta1=0.9, beta2=0.999, eps=1e-8, grad_scale=1.0):
    require_gpu(p, g, m, v, seg_end, seg_group, group_lr)
    _check(lib().a4r_adam_step(_stream(), _p(p), _p(g), _p(m), _p(v), p.numel(), _p(seg_end), _p(seg_group), seg_end.numel(), _p(group_lr), step, beta1, beta2, eps, grad_scale),
           'a4r_adam_step')


def _need(cond, what):
    if not cond:
        raise ValueError(what)


def grad_sumsq(g, partials, grad_scale=1.0):
    """a4r_grad_sumsq: partials (fp64 [GRAD_NORM_PARTS]) = the fixed-order fp64 partial sums of (g * grad_scale)^2 that a4r_adamw_step clips
    with.  g is read with 16-byte loads when it is 16-byte aligned; the partials do not depend on that."""
    _need(g.dtype == torch.float32 and g.is_contiguous() and g.numel() > 0, 'grad_sumsq: g must be a non-empty contiguous fp32 tensor')
    _need(partials.dtype == torch.float64 and partials.is_contiguous() and partials.numel() == GRAD_NORM_PARTS,
          f'grad_sumsq: partials must be contiguous fp64 with {GRAD_NORM_PARTS} elements')
    require_gpu(g, partials)
    _check(lib().a4r_grad_sumsq(_stream(), _p(g), g.numel(), grad_scale, _p(partials)), 'a4r_grad_sumsq')


def adamw_step(p, g, m, v, seg_end, seg_group, group_lr, group_wd, step, beta1=0.9, beta2=0.999, eps=1e-8, grad_scale=1.0, decoupled=True,
               partials=None, max_norm=0.0, norm_out=None):
    """a4r_adamw_step: Adam with per-group weight decay group_wd (decoupled: AdamW, else torch Adam's coupled form) and, when partials (grad_sumsq of
    this g) is given, the gradient clipped to max_norm with the pre-clip norm stored into norm_out (a one-element fp32 tensor, optional).  The quad
    kernel runs when n >= 2^20 and p, g, m, v are 16-byte aligned; the results are the same either way.  Argument errors raise ValueError before
    the call."""
    n = p.numel()
    for name, t in (('p', p), ('g', g), ('m', m), ('v', v)):
        _need(t.dtype == torch.float32 and t.is_contiguous() and t.numel() == n and n > 0,
              f'adamw_step: {name} must be a contiguous fp32 tensor of p\'s {n} (> 0) elements')
    for name, t in (('seg_end', seg_end), ('seg_group', seg_group)):
        _need(t.dtype == torch.int32 and t.is_contiguous(), f'adamw_step: {name} must be contiguous int32')
    _need(seg_end.numel() == seg_group.numel() > 0, 'adamw_step: seg_end and seg_group must hold the same number (> 0) of segments')
    for name, t in (('group_lr', group_lr), ('group_wd', group_wd)):
        _need(t.dtype == torch.float32 and t.is_contiguous(), f'adamw_step: {name} must be contiguous fp32')
    _need(group_lr.numel() == group_wd.numel(), 'adamw_step: group_lr and group_wd must hold one value per group')
    _need(int(step) >= 1, 'adamw_step: step counts from 1')
    if partials is not None:
        _need(partials.dtype == torch.float64 and partials.is_contiguous() and partials.numel() == GRAD_NORM_PARTS,
              f'adamw_step: partials must be contiguous fp64 with {GRAD_NORM_PARTS} elements')
        _need(math.isfinite(max_norm) and max_norm > 0, f'adamw_step: max_norm must be a finite positive number, got {max_norm}')
    if norm_out is not None:
        _need(partials is not None, 'adamw_step: norm_out needs partials (the norm exists only when clipping)')
        _need(norm_out.dtype == torch.float32 and norm_out.numel() == 1, 'adamw_step: norm_out must be a one-element fp32 tensor')
    require_gpu(p, g, m, v, seg_end, seg_group, group_lr, group_wd, partials, norm_out)
    _check(lib().a4r_adamw_step(_stream(), _p(p), _p(g), _p(m), _p(v), n, _p(seg_end), _p(seg_group), seg_end.numel(), _p(group_lr), int(step), beta1, beta2, eps, grad_scale,
                                _p(group_wd), int(bool(decoupled)), _p(partials), max_norm if partials is not None else 0.0, _p(norm_out)), 'a4r_adamw_step')


def pack_matrices(flat, desc_dev, n_desc, max_elems, dtype):
    _check(lib().a4r_pack_matrices(_stream(), _p(flat), _p(desc_dev), n_desc, max_elems, dtype), 'a4r_pack_matrices')


def topk_ws_bytes(U, N1, k):
    """Bytes of a4r_topk_items' workspace (a host-side query, no GPU); 0 for a shape the kernel refuses."""
    return int(lib().a4r_topk_ws_bytes(U, N1, k))


def topk_items(prec, item_emb, excl_ptr, excl_idx, k, ids, scores):
    """a4r_topk_items: ids [U, k] int32 / scores [U, k] fp32 = the k best items 1 .. N1-1 of every user, excluding the user's CSR list
    excl_idx[excl_ptr[u] .. excl_ptr[u + 1]) (<= EVAL_MAX_HISTORY ids each: the caller checks, as for eval_rank), by score descending, ties by
    smaller id; short lists end in id 0 / -inf (include/a4r.h).  The workspace is allocated here."""
    require_gpu(prec, item_emb, excl_ptr, excl_idx, ids, scores)
    U, N1, E = _sweep_operands('topk_items', torch.float32, prec, item_emb)
    k, excl_idx, ws = _topk_args('topk_items', prec.device, U, excl_ptr, excl_idx, k, ids, scores, lambda k: topk_ws_bytes(U, N1, k))
    _check(lib().a4r_topk_items(_stream(), _p(prec), _p(item_emb), _p(excl_ptr), _p(excl_idx), _p(ids), _p(scores), _p(ws), U, N1, E, k), 'a4r_topk_items')
    return ids, scores


def _sweep_operands(what, dtype, prec, table):
    """The operands of an item-table sweep, prec [U, E] and the table [N1, E], checked for the wrapper `what` (topk_items, topk_items_cand: fp32;
    topk_items_bf16, eval_rank_bf16: bf16, under their own names) -> U, N1, E.  A wrapper
    with a candidate mask checks it behind this, once N1 stands, and in front of _topk_args."""
    a, b, spelt = ('prec', 'item_emb', 'fp32') if dtype == torch.float32 else ('prec_b', 'table_b', 'bf16 (the copies cast_bf16 writes)')
    if prec.dim() != 2 or table.dim() != 2 or prec.shape[1] != table.shape[1]:
        raise ValueError(f'{what}: {a} [U, E] and {b} [N1, E] expected, got {tuple(prec.shape)} and {tuple(table.shape)}')
    U, E = prec.shape
    N1 = table.shape[0]
    if prec.dtype != dtype or table.dtype != dtype or not prec.is_contiguous() or not table.is_contiguous():
        raise ValueError(f'{what}: {a} and {b} must be contiguous {spelt}')
    if E not in TOPK_E:
        raise ValueError(f'{what}: E = {E}, supported {TOPK_E}')
    if U < 1 or N1 < 2:
        raise ValueError(f'{what}: U = {U} users and N1 = {N1} table rows (row 0 = the pad item): need U >= 1, N1 >= 2')
    if (prec.data_ptr() | table.data_ptr()) & 15:
        raise ValueError(f'{what}: {a} and {b} must be 16-byte aligned')
    return U, N1, E


def _topk_k(what, k):
    k = int(k)
    if not 1 <= k <= TOPK_MAX_K:
        raise ValueError(f'{what}: k = {k} outside 1 .. {TOPK_MAX_K}')
    return k


def _topk_outputs(what, rows, k, ids, scores, f32='fp32'):
    """The outputs of a top-K wrapper: ids int32 / scores fp32 (spelt f32 in the wrapper's messages), contiguous [rows, k]"""
    if ids.dtype != torch.int32 or not ids.is_contiguous():
        raise ValueError(f'{what}: ids must be contiguous int32')
    if scores.dtype != torch.float32 or not scores.is_contiguous():
        raise ValueError(f'{what}: scores must be contiguous {f32}')
    if tuple(ids.shape) != (rows, k) or tuple(scores.shape) != (rows, k):
        raise ValueError(f'{what}: ids and scores must be [{rows}, {k}]')


def _topk_args(what, device, U, excl_ptr, excl_idx, k, ids, scores, ws_bytes):
    """What topk_items, topk_items_cand and topk_items_bf16 do between their operand checks and their call: the checks of k, the CSR exclusion
    lists and the outputs, a stand-in for an empty excl_idx, the workspace of ws_bytes(k) bytes (the wrapper's own query) -> k, excl_idx, ws"""
    k = _topk_k(what, k)
    for name, t in (('excl_ptr', excl_ptr), ('excl_idx', excl_idx)):
        if t.dtype != torch.int32 or not t.is_contiguous():
            raise ValueError(f'{what}: {name} must be contiguous int32')
    if excl_ptr.numel() != U + 1:
        raise ValueError(f'{what}: excl_ptr must hold U + 1 = {U + 1} offsets, got {excl_ptr.numel()}')
    _topk_outputs(what, U, k, ids, scores)
    if excl_idx.numel() == 0:                 # (an empty list has no data pointer; the kernel reads no id of it)
        excl_idx = torch.zeros(1, dtype=torch.int32, device=device)
    return k, excl_idx, torch.empty(ws_bytes(k), dtype=torch.uint8, device=device)


def eval_rank(prec, item_emb, target, hist_ptr, hist_idx, rank):
    require_gpu(prec, item_emb, target, hist_ptr, hist_idx, rank)
    _check(lib().a4r_eval_rank(_stream(), _p(prec), _p(item_emb), _p(target), _p(hist_ptr), _p(hist_idx), _p(rank), prec.shape[0], item_emb.shape[0], prec.shape[1]),
           'a4r_eval_rank')


def id_sample(seqs, rows, item_num, seed, draw, negatives, ids, log_mask, err):
    """a4r_id_sample: the training batch of the users rows [B] (int32 rows of seqs, int32 [n_users, L] left-padded with 0) -> ids int64 [B, L, 2]
    (positives | one negative per real position except the last), log_mask fp32 [B, L - 1], err int32 [1] (out-of-range rows and users without a
    candidate, overwritten).  The negative of (user row, position) is a pure function of (seed, draw, row, position) (include/a4r.h);
    negatives false: column 1 stays 0 and nothing is drawn.  Argument errors raise ValueError before the call."""
    for name, t in (('seqs', seqs), ('rows', rows), ('err', err)):
        if t.dtype != torch.int32 or not t.is_contiguous():
            raise ValueError(f'id_sample: {name} must be contiguous int32')
    if seqs.dim() != 2 or rows.dim() != 1:
        raise ValueError(f'id_sample: seqs [n_users, L] and rows [B] expected, got {tuple(seqs.shape)} and {tuple(rows.shape)}')
    n_users, L = seqs.shape
    B = rows.numel()
    if not 2 <= L <= SAMPLE_MAX_L:
        raise ValueError(f'id_sample: L = {L} outside 2 .. {SAMPLE_MAX_L}')
    if B < 1 or n_users < 1 or not 1 <= int(item_num) < 2 ** 31:
        raise ValueError(f'id_sample: B = {B} rows, n_users = {n_users}, item_num = {item_num}: need B >= 1, n_users >= 1, 1 <= item_num < 2^31')
    if not 0 <= int(draw) < 2 ** 24:
        raise ValueError(f'id_sample: draw = {draw} outside 0 .. 2^24 - 1')
    if ids.dtype != torch.int64 or not ids.is_contiguous() or tuple(ids.shape) != (B, L, 2):
        raise ValueError(f'id_sample: ids must be contiguous int64 [{B}, {L}, 2]')
    if log_mask.dtype != torch.float32 or not log_mask.is_contiguous() or tuple(log_mask.shape) != (B, L - 1):
        raise ValueError(f'id_sample: log_mask must be contiguous fp32 [{B}, {L - 1}]')
    if err.numel() != 1:
        raise ValueError('id_sample: err must hold one int32')
    require_gpu(seqs, rows, ids, log_mask, err)
    _check(lib().a4r_id_sample(_stream(), _p(seqs), n_users, L, _p(rows), B, int(item_num), int(seed) & (2 ** 64 - 1), int(draw), int(bool(negatives)), _p(ids), _p(log_mask),
                               _p(err)), 'a4r_id_sample')


# Exports declared in a header of their own (which include/a4r.h includes) and bound in a satellite module with a signature table of its own, which
# lib() above checks and installs at load beside SIGNATURES.  A satellite's table, wrappers and constants are reachable under this module's name as
# well; they are resolved on first use, so either module can be imported first.  This is the one place a satellite is listed:
#   module: (its signature table, the other names reachable here)
SATELLITES = {
    # the cross-entropy head on the bf16 MFMA (--ce_dtype bf16): include/a4r_score_ce_bf16.h
    '_lib_ce_bf16': ('SCORE_CE_BF16_SIGNATURES', ('SCORE_CE_BF16_E', 'SCORE_CE_BF16_ROWS', 'cast_bf16', 'score_ce_bf16_bwd', 'score_ce_bf16_fwd',
                                                  'score_ce_bf16_ranges', 'score_ce_bf16_ws_bytes')),
    # evaluation and top-K within a candidate set of items: include/a4r_candidates.h
    '_lib_candidates': ('CANDIDATES_SIGNATURES', ('candidate_mask', 'eval_rank_cand', 'topk_items_cand')),
    # top-K and rank within a candidate list of each user's own: include/a4r_user_lists.h
    '_lib_user_lists': ('USER_LISTS_SIGNATURES', ('LIST_MAX', 'topk_lists', 'eval_rank_lists')),
    # the negatives of a sampled evaluation drawn on the device: include/a4r_eval_negatives.h
    '_lib_eval_negatives': ('EVAL_NEGATIVES_SIGNATURES', ('EVAL_NEG_SITE', 'EVAL_NEG_MAX', 'eval_draw_negatives', 'eval_rank_sampled')),
    # the diversified re-ranking of a top-K list: include/a4r_diversify.h
    '_lib_diversify': ('DIVERSIFY_SIGNATURES', ('MMR_MAX_POOL', 'mmr_rerank')),
    # similar items, every query item's nearest items of the table: include/a4r_similar.h
    '_lib_similar': ('SIMILAR_SIGNATURES', ('row_inv_norms', 'topk_similar')),
    # evaluation and top-K with scores from the bf16 MFMA (--score_dtype bf16): include/a4r_score_bf16.h
    '_lib_score_bf16': ('SCORE_BF16_SIGNATURES', ('eval_rank_bf16', 'topk_items_bf16', 'topk_bf16_ws_bytes')),
    # audience lists, every query item's best users of a user table: include/a4r_audience.h
    '_lib_audience': ('AUDIENCE_SIGNATURES', ('topk_users',)),
    # top-K with exclusion lists of any length, read from global memory: include/a4r_exclude.h
    '_lib_exclude': ('EXCLUDE_SIGNATURES', ('topk_items_excl',)),
}


def __getattr__(name):
    for module, (table, names) in SATELLITES.items():
        if name == table or name in names:
            return getattr(importlib.import_module('.' + module, __package__), name)
    raise AttributeError(f'module {__name__!r} has no attribute {name!r}')
