"""Build-time records of the engines (engine.py, engine_vit.py): what one LayerNorm, adapter, LoRA, backbone Linear, transformer block or
K-Adapter carries on the device -- kernel-side operand copies, gradient sinks, geometry.  They are filled once while an engine is built and only
read afterwards.  `eng` is the engine under construction; the records use it through grad_view, scratch, add_corner, add_pack, add_pack_bias,
add_virtual, dev and _f32 only, and the ORDER of those calls fixes the pack tables, the scratch arena layout and the corner table.
"""
import math

import torch

from . import _lib as L
from .model.modules import HyperComplexAdapterBlock


def pad_to(n, m):
    return (n + m - 1) // m * m


class _LN:
    """LayerNorm parameters (fp32) + optional gradient sinks."""

    def __init__(self, mod, eng):
        self.gamma, self.beta, self.eps = mod.weight, mod.bias, mod.eps
        self.g_gamma = eng.grad_view(mod.weight)
        self.g_beta = eng.grad_view(mod.bias)


class _Adapter:
    """One bottleneck adapter: kernel-side copies (compute dtype, bottleneck padded to 64) + gradient sinks."""
    parallel = False             # image tower: the adapter reads the sub-layer INPUT (set by ViTRecEngine._vit_so; the text tower keeps placements on the block)

    def __init__(self, mod, width, eng, dt):
        self.kind = mod.kind
        self.act = L.ACT_BY_NAME[mod.activation_name]
        dev = eng.dev
        if isinstance(mod, HyperComplexAdapterBlock):
            self.d = mod.down_sampler.out_features
            self.virtual = (mod.down_sampler, mod.up_sampler)
            b_down, b_up = mod.down_sampler.b, mod.up_sampler.b
            for lin in self.virtual:     # gradients of these arrive through _virtual_backward
                for q in (lin.W_left, lin.W_right, lin.phm_rule):
                    if q is not None:
                        eng.grad_view(q)
        else:
            self.d = mod.fc_down.out_features
            self.virtual = None
            self.p_wd, self.p_wu = mod.fc_down.weight, mod.fc_up.weight
            b_down, b_up = mod.fc_down.bias, mod.fc_up.bias
        self.dp = pad_to(self.d, 64)
        self.width = width
        self.wd = torch.zeros(self.dp, width, dtype=dt, device=dev)      # fc_down.weight  [d, H]
        self.wdT = torch.zeros(width, self.dp, dtype=dt, device=dev)
        self.wu = torch.zeros(width, self.dp, dtype=dt, device=dev)      # fc_up.weight    [H, d]
        self.wuT = torch.zeros(self.dp, width, dtype=dt, device=dev)
        self.p_bd, self.p_bu = b_down, b_up
        self.bd = torch.zeros(self.dp, dtype=torch.float32, device=dev)  # padded copy of fc_down.bias
        self.bu = b_up                                                   # [H] fp32, used in place
        self.g_bu = eng.grad_view(b_up)
        self.g_bd = eng.grad_view(b_down)
        self.g_wd = self.g_wu = None
        # the same four matrices in the FRAGMENT order of the one-launch adapter kernels (a4r_pack_matrices layouts 1 / 2, include/a4r.h: every wave
        # instruction of those kernels' prologues then reads 1 KiB contiguous; the first tile of a launch starts ~3 us earlier).  Row-major copies stay:
        # the three-launch forms, the weight-gradient kernels' shapes and the tests read them.  (fwd: wd, wu; bwd: wuT, wdT)
        self.frag_f = self.frag_b = None
        if dt == torch.bfloat16 and self.dp == 64 and width in (128, 256, 512, 768, 1024):
            mk = lambda: torch.zeros(64 * width, dtype=dt, device=dev)
            self.frag_f, self.frag_b = (mk(), mk()), (mk(), mk())
        if self.virtual is None:
            self.g_wd, self.g_wu = eng.grad_view(self.p_wd), eng.grad_view(self.p_wu)
            eng.add_pack(self.p_wd, self.wd, False)
            eng.add_pack(self.p_wd, self.wdT, True)
            eng.add_pack(self.p_wu, self.wu, False)
            eng.add_pack(self.p_wu, self.wuT, True)
            if self.frag_f is not None:
                for p_, dst, code in self.frag_entries():
                    eng.add_pack(p_, dst, code)
        else:
            eng.add_virtual(self)
        eng.add_pack_bias(b_down, self.bd)
        # scratch for padded weight gradients (used when d < dp, or for virtual matrices)
        direct = self.virtual is None and self.d == self.dp
        self.s_wd = None if direct else eng.scratch(self.dp, width)
        self.s_wu = None if direct else eng.scratch(width, self.dp)
        self.s_bd = None if self.d == self.dp else eng.scratch(1, self.dp)[0]
        if self.virtual is None and not direct:          # the valid corners go into the flat gradient at the end of backward
            eng.add_corner(self.s_wu, self.p_wu, width, self.d)
            eng.add_corner(self.s_wd, self.p_wd, self.d, width)
        if self.s_bd is not None:
            eng.add_corner(self.s_bd.view(1, -1), b_down, 1, self.d)

    def frag_entries(self, wd_src=None, wu_src=None):
        """(source, destination, a4r_pack_desc_t.transpose code) of the four fragment-ordered copies: bit 0 transpose, bits 1-2 layout (1: [64, H], 2: [H, 64]);
        destinations are viewed with their LOGICAL shape so that the descriptor carries rows_pad / cols_pad"""
        wd_src = self.p_wd if wd_src is None else wd_src
        wu_src = self.p_wu if wu_src is None else wu_src
        W = self.width
        return [(wd_src, self.frag_f[0].view(64, W), 2), (wu_src, self.frag_f[1].view(W, 64), 4),
                (wu_src, self.frag_b[0].view(64, W), 2 | 1), (wd_src, self.frag_b[1].view(W, 64), 4 | 1)]


class _Lora:
    """LoRA on one projection (q or v) of a fused qkv weight: W_eff = W + B A / r is re-merged into the packed qkv operand
    every step (so forward and dgrad cost nothing extra); the low-rank gradients come from four skinny products in backward:
    t = x A^T, dt = (dq B) s, dB = dq^T t s, dA = dt^T x."""

    ONES_COL = 32            # (shared form: rank columns 0 - 7 and 16 - 23 are in use)

    def __init__(self, mod, width, eng, dt, slot, share=None):
        """share = (dict, off): this LoRA is one of a block's two small-rank ones (r <= 16: the image tower's q, v at r = 8).  They then use
        ONE [64, width] A operand (rank rows at off .. off + r), ONE t = x A^T and ONE dA = dt^T x launch; only the products that read
        this projection's own gradient (dt = dq B, dB = dq^T t, the bias sum) stay per LoRA.  The rank was padded to 64 columns anyway."""
        self.mod, self.slot, self.width = mod, slot, width
        self.r, self.rp, self.scaling = mod.r, pad_to(mod.r, 64), float(mod.scaling)
        dev = eng.dev
        self.g_bias = eng.grad_view(mod.bias) if mod.bias is not None else None
        self.g_W = None
        self.share = None
        if self.r == 0:                  # loralib: r = 0 leaves a plain Linear whose weight stays trainable (CV run_adapter.py:394)
            self.g_W = eng.grad_view(mod.weight)
            return
        self.g_A, self.g_B = eng.grad_view(mod.lora_A), eng.grad_view(mod.lora_B)
        self.BT = torch.zeros(self.rp, width, dtype=dt, device=dev)       # lora_B^T [r, out]     (NT operand of dt = dq B)
        self.s_B = eng.scratch(width, self.rp)
        if share is not None:
            sh, off = share
            self.share, self.off = sh, off
            if 'A' not in sh:
                sh['A'] = torch.zeros(self.rp, width, dtype=dt, device=dev)
                sh['s_A'] = eng.scratch(self.rp, width)
            self.A, self.s_A = sh['A'], sh['s_A']
            eng.add_pack(mod.lora_A, sh['A'][off:off + 16], False)                   # rows off .. off + r (zero-padded to 16)
            eng.add_pack(mod.lora_B, self.BT[off:off + 16], True)                    # B^T at the same rank rows: dt lands in columns off .. off + r
            eng.add_corner(self.s_B[:, off:off + 16], mod.lora_B, width, self.r, alpha=self.scaling)
            eng.add_corner(sh['s_A'][off:off + 16], mod.lora_A, self.r, width)
            # the bias gradient (column sums of this projection's gradient) rides in the dB product: column ONES_COL of t is a column of
            # ones (a bias of the t = x A^T launch: row ONES_COL of A is zero), so (dq^T t)[:, ONES_COL] = sum over rows of dq
            if 'ones' not in sh:
                sh['ones'] = torch.zeros(self.rp, dtype=torch.float32, device=dev)
                sh['ones'][self.ONES_COL] = 1.0
            if self.g_bias is not None:
                eng.add_corner(self.s_B[:, self.ONES_COL:self.ONES_COL + 1], mod.bias, width, 1)
            return
        self.A = torch.zeros(self.rp, width, dtype=dt, device=dev)        # lora_A [r, in]        (NT operand of t = x A^T)
        eng.add_pack(mod.lora_A, self.A, False)
        eng.add_pack(mod.lora_B, self.BT, True)
        self.s_A = eng.scratch(self.rp, width)
        eng.add_corner(self.s_B, mod.lora_B, width, self.r, alpha=self.scaling)      # dB = (dq^T t) s
        eng.add_corner(self.s_A, mod.lora_A, self.r, width)

    @classmethod
    def for_block(cls, lins, width, eng, dt):
        """The _Lora objects of a block's (query, key, value) projections; two small-rank ones share their A-side launches."""
        idx = [i for i, lin in enumerate(lins) if type(lin).__name__ == 'LoRALinear']
        small = [i for i in idx if 0 < lins[i].r <= 16]
        share = {} if (len(small) == 2 and len(idx) == 2) else None
        out = []
        for i in idx:
            out.append(cls(lins[i], width, eng, dt, i, share=(share, 16 * small.index(i)) if share is not None else None))
        return out


class _Dense:
    """One Linear of the backbone: compute-dtype copies W [out, in] (NT operand) and W^T (dgrad operand).  Frozen: filled once.
    Trainable (--fine_tune_to all, Pretraining/): the copies are re-packed from the flat fp32 master every step and g_w / g_b
    receive dW = dY^T X (a4r_gemm_tn) and db = column sums of dY (a4r_colsum)."""

    def __init__(self, eng, weight, bias, dt, w_dst=None, wT_dst=None, b_dst=None, view2d=None, pad=None):
        out_f, in_f = view2d if view2d is not None else weight.shape          # view2d: a Conv2d weight seen as [out, C*kh*kw]
        op, ip = pad if pad is not None else (out_f, in_f)                     # pad: zero-padded storage (K-Adapter blocks 16 -> 64 wide)
        self.view2d, self.out_f, self.in_f = view2d, out_f, in_f
        self.w = w_dst if w_dst is not None else torch.zeros(op, ip, dtype=dt, device=eng.dev)
        self.wT = wT_dst if wT_dst is not None else torch.zeros(ip, op, dtype=dt, device=eng.dev)
        padded = tuple(self.w.shape) != (out_f, in_f)
        if weight.requires_grad:
            eng.add_pack(weight, self.w, False)
            eng.add_pack(weight, self.wT, True)
        else:
            w2 = weight.detach().reshape(out_f, in_f)
            self.w[:out_f, :in_f].copy_(w2.to(dt))
            self.wT[:in_f, :out_f].copy_(w2.t().to(dt))
        self.g_w = eng.grad_view(weight)
        self.s_w = eng.scratch(*self.w.shape) if (padded and self.g_w is not None) else None
        if self.s_w is not None:
            eng.add_corner(self.s_w, weight, out_f, in_f)
        self.b = self.g_b = self.s_b = None
        if bias is not None:
            if b_dst is None and padded:
                b_dst = torch.zeros(self.w.shape[0], dtype=torch.float32, device=eng.dev)
            if b_dst is not None:
                self.b = b_dst
                if bias.requires_grad:
                    eng.add_pack_bias(bias, b_dst[:out_f])
                else:
                    b_dst[:out_f].copy_(bias.detach().float())
            else:
                self.b = bias.data if bias.requires_grad else eng._f32(bias)     # trainable: the fp32 master (a flat_p view) itself
            self.g_b = eng.grad_view(bias)
            if padded and self.g_b is not None:
                self.s_b = eng.scratch(1, self.w.shape[0])[0]
                eng.add_corner(self.s_b.view(1, -1), bias, 1, out_f)
        self.trainable = self.g_w is not None or self.g_b is not None


class _Block:
    """One transformer block with optional adapters: a post-LN BERT layer, SASRec block or K-Adapter block (ln1 / ln2), or a pre-LN ViT
    layer (lnA / lnB).  Every field a block can carry is declared here; assigning any other name raises.

    Built in two calls because the order of the engine's bookkeeping calls is part of the layout (module docstring): the constructor does
    the q / k / v side, the caller then unwraps its two output modules (which builds their adapters and new LayerNorms), set_dense() does
    the three Linears, and the caller finishes with the LayerNorms and what is its own (dropout, sites, placements, need_dx, is_item)."""
    __slots__ = ('H', 'Hv', 'F', 'nh', 'dh', 'S', 'T', 'scale', 'ffn_act', 'long', 'is_item', 'causal', 'mask_neg', 'p_hidden', 'p_attn', 'site',
                 'need_dx', 'lora', 'wqkv', 'wqkvT', 'bqkv', 'qkv', 'd_o', 'd_i', 'd_o2', 'train_dense',
                 'wo', 'woT', 'bo', 'wi', 'wiT', 'bi', 'wo2', 'wo2T', 'bo2',
                 'ln1', 'ln2', 'lnA', 'lnB', 'ad1', 'ad2', 'pl1', 'pl2', 'lnn1', 'lnn2',
                 'wqkv8', 'wqkv8s', 'wi8', 'wi8s', 'wo8', 'wo8s', 'wo28', 'wo28s', 'wo2T8', 'wo2T8s', 'wiT8', 'wiT8s', 'wqkv8_dyn', 'c_du',
                 'vskip_ok')

    def __init__(self, eng, proj, H, Hv, F, nh, S, dt, qkv_bias, ffn_act):
        """proj: the (query, key, value) modules, Linear or LoRALinear.  H / F: storage widths (multiples of 64), Hv <= H: the valid width
        (K-Adapter blocks: 16 stored zero-padded to 64; the LayerNorms run on the valid columns only).  qkv_bias: the projections carry
        biases (BERT, ViT); without, the fused bias exists only for LoRA (lora.Linear carries one)."""
        for lin in proj:
            if type(lin).__name__ not in ('LoRALinear', 'Linear'):
                raise NotImplementedError(f'projection module {type(lin).__name__}')
        self.lora = _Lora.for_block(proj, Hv, eng, dt)
        if self.lora and H != Hv:
            raise NotImplementedError('LoRA on a zero-padded block')
        self.H, self.Hv, self.F, self.nh, self.dh, self.S, self.T = H, Hv, F, nh, Hv // nh, S, dt
        self.scale, self.ffn_act = 1.0 / math.sqrt(self.dh), ffn_act
        self.long = self.is_item = self.causal = False      # long: a4r_attn_long_* with the key mask; is_item: a block of the item tower (follows the engine's _pk)
        self.mask_neg = self.p_hidden = self.p_attn = 0.0
        self.site, self.need_dx = 0, True
        self.ln1 = self.ln2 = self.lnA = self.lnB = None                                          # post-LN pair or pre-LN pair
        self.ad1 = self.ad2 = self.pl1 = self.pl2 = self.lnn1 = self.lnn2 = None                  # adapter, placement, Pfeiffer's new LayerNorm per half
        # e4m3 operands + per-output-channel scales of the frozen Linears (TransRecEngine._build_fp8); None: that GEMM stays bf16
        self.wqkv8 = self.wqkv8s = self.wi8 = self.wi8s = self.wo8 = self.wo8s = self.wo28 = self.wo28s = None
        self.wo2T8 = self.wo2T8s = self.wiT8 = self.wiT8s = self.c_du = None
        self.wqkv8_dyn = False                              # wqkv8 is re-quantised after every LoRA merge
        self.vskip_ok = {'1': None, '2': None}              # TransRecEngine._vskip's verdict per half, None = not decided yet (it reads the LayerNorm back)
        dev = eng.dev
        self.wqkv = torch.zeros(3 * H, H, dtype=dt, device=dev)
        self.wqkvT = torch.zeros(H, 3 * H, dtype=dt, device=dev)
        self.bqkv = torch.zeros(3 * H, dtype=torch.float32, device=dev) if (qkv_bias or self.lora) else None
        sl_ = lambda sl: slice(sl * H, (sl + 1) * H)
        for lo in self.lora:       # lora.Linear keeps a (trainable) bias: its fp32 master is copied into the fused qkv bias by the per-step pack launch
            if lo.mod.bias is not None:
                eng.add_pack_bias(lo.mod.bias, self.bqkv[sl_(lo.slot)])
        self.qkv = tuple(None if type(lin).__name__ == 'LoRALinear' else          # LoRA slots are merged in pack_trainables
                         _Dense(eng, lin.weight, lin.bias if qkv_bias else None, dt, self.wqkv[sl_(sl)], self.wqkvT[:, sl_(sl)],
                                self.bqkv[sl_(sl)] if qkv_bias else None)
                         for sl, lin in enumerate(proj))

    def set_dense(self, eng, o, i, o2):
        """The attention-output, FFN-up and FFN-down Linears.  wo .. bo2 are plain fields on purpose: the step reads them ~400 times."""
        H, F, dt = self.H, self.F, self.T
        self.d_o = _Dense(eng, o.weight, o.bias, dt, pad=(H, H))
        self.d_i = _Dense(eng, i.weight, i.bias, dt, pad=(F, H))
        self.d_o2 = _Dense(eng, o2.weight, o2.bias, dt, pad=(H, F))
        self.wo, self.woT, self.bo = self.d_o.w, self.d_o.wT, self.d_o.b
        self.wi, self.wiT, self.bi = self.d_i.w, self.d_i.wT, self.d_i.b
        self.wo2, self.wo2T, self.bo2 = self.d_o2.w, self.d_o2.wT, self.d_o2.b
        # any backbone Linear of the block trainable (--fine_tune_to all)
        self.train_dense = any(d is not None and d.trainable for d in self.qkv + (self.d_o, self.d_i, self.d_o2))


class _KAdapter:
    """Engine side of one KAdapterBlock (modules.py:161-206): down (trainable Linear) -> two plain post-LN blocks (all weights
    trainable, no mask, not causal) -> up, + input."""
    __slots__ = ('width', 'd', 'dp', 'T', 'down', 'up', 'blocks', 'tag')
