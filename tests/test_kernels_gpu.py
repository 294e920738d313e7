"""GPU: every C-ABI kernel against a plain torch fp32 reference of the same op (per-kernel parity).

fp32 instantiations are held to 1e-4-class tolerances (they are exact fp32 MFMA chains); bf16
instantiations to bf16-rounding tolerances (inputs are pre-rounded to bf16 so only accumulation
order and the output rounding differ).
"""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

DT = {'bf16': torch.bfloat16, 'f32': torch.float32}


def dev():
    return torch.device('cuda:0')


def rnd(*shape, dtype=torch.float32, scale=1.0, seed=None):
    g = torch.Generator(device='cpu')
    g.manual_seed(seed if seed is not None else sum(shape) * 7919 + len(shape))
    return (torch.randn(*shape, generator=g) * scale).to(dtype).to(dev())


def close(got, ref, dtype, what, atol32=2e-4, rtol32=2e-4, atol16=None, rtol16=3e-2):
    got = got.float().cpu()
    ref = ref.float().cpu()
    assert torch.isfinite(got).all(), f'{what}: non-finite output'
    if dtype == torch.float32:
        atol, rtol = atol32, rtol32
    else:
        atol = atol16 if atol16 is not None else 3e-2 * max(1.0, float(ref.abs().max()))
        rtol = rtol16
    err = (got - ref).abs()
    lim = atol + rtol * ref.abs()
    bad = err > lim
    assert not bad.any(), (f'{what}: {int(bad.sum())}/{bad.numel()} out of tolerance, max err {float(err.max()):.3e} '
                           f'(ref max {float(ref.abs().max()):.3e}) first bad idx {bad.nonzero()[0].tolist()}')


def act_ref(x, act):
    if act == 1:
        return torch.relu(x)
    if act == 2:
        return torch.nn.functional.gelu(x)
    if act == 3:
        return torch.nn.functional.gelu(x, approximate='tanh')
    if act == 4:
        return torch.nn.functional.leaky_relu(x, 0.01)
    return x


# ------------------------------------------------------------------ GEMM NT
@pytest.fixture(params=[4, 2, 1, 0], ids=['tile256', 'auto', 'glds', 'regstage'])
def gemm_variant(request):
    from adapter4rec_amd import _lib as L
    old = L.gemm_variant(request.param)
    yield request.param
    L.gemm_variant(old)


@pytest.mark.parametrize('dt', ['f32', 'bf16'])
@pytest.mark.parametrize('M,N,K', [(128, 64, 64), (256, 128, 128), (384, 768, 768), (256, 2304, 768), (128, 192, 3072), (256, 64, 768),
                                   (128, 128, 192), (128, 64, 320), (256, 256, 128), (512, 768, 768), (256, 256, 192),
                                   (768, 2304, 768), (256, 768, 3072), (256, 3072, 64)])
def test_gemm_plain(dt, M, N, K, gemm_variant):
    from adapter4rec_amd import _lib as L
    t = DT[dt]
    A, B = rnd(M, K, dtype=t, seed=1), rnd(N, K, dtype=t, scale=0.05, seed=2)
    Cc = torch.zeros(M, N, dtype=t, device=dev())
    L.gemm_nt(A, B, Cc)
    close(Cc, A.float() @ B.float().t(), t, f'gemm {dt} {M}x{N}x{K}')


def test_gemm_identity_asymmetric(gemm_variant):
    """A = I with an asymmetric B catches swapped row/col maps (guide section 3)."""
    from adapter4rec_amd import _lib as L
    n = 256
    for t in (torch.float32, torch.bfloat16):
        A = torch.zeros(n, n, dtype=t, device=dev())
        A[:, :] = torch.eye(n)
        B = (torch.arange(n * n, dtype=torch.float32).view(n, n) % 251 - 125).to(t).to(dev())   # small ints: exact in bf16
        Cc = torch.zeros(n, n, dtype=t, device=dev())
        L.gemm_nt(A, B, Cc)
        assert torch.equal(Cc.float().cpu(), B.float().t().cpu())


@pytest.mark.parametrize('dt', ['f32', 'bf16'])
def test_gemm_epilogue_full(dt, gemm_variant):
    from adapter4rec_amd import _lib as L
    t = DT[dt]
    M, N, K = (256, 256, 192) if gemm_variant >= 2 else (256, 192, 128)
    A, B = rnd(M, K, dtype=t, seed=3), rnd(N, K, dtype=t, scale=0.1, seed=4)
    bias = rnd(N, seed=5)
    R1, R2, Pre = rnd(M, N, dtype=t, seed=6), rnd(M, N, dtype=t, seed=7), rnd(M, N, dtype=t, seed=8)
    for act, dact, c2d in [(0, 0, 0), (1, 0, 0), (2, 0, 0), (3, 0, 0), (0, 2, 0), (0, 1, 0), (4, 3, 0), (2, 0, 1), (1, 0, 1), (0, 15, 0)]:
        Cc = torch.zeros(M, N, dtype=t, device=dev())
        C2 = torch.zeros(M, N, dtype=t, device=dev())
        L.gemm_nt(A, B, Cc, bias=bias, C2=C2, R1=R1, R2=R2, Pre=Pre, act=act, dact=dact, alpha=0.5, c2_deriv=bool(c2d))
        pre = 0.5 * (A.float() @ B.float().t()) + bias
        ref = act_ref(pre, act)
        if dact == 15:
            ref = ref * Pre.float()
        elif dact:
            p = Pre.float().clone().requires_grad_(True)
            act_ref(p, dact).sum().backward()
            ref = ref * p.grad
        ref = ref + R1.float() + R2.float()
        if c2d:
            q = pre.clone().requires_grad_(True)
            act_ref(q, act).sum().backward()
            close(C2, q.grad, t, f'gemm C2 = act\'(pre) act={act}')
        else:
            close(C2, pre, t, f'gemm C2 act={act}')
        close(Cc, ref, t, f'gemm epilogue act={act} dact={dact}')


@pytest.mark.parametrize('M,N,K', [(256, 256, 192), (512, 3072, 768), (128, 192, 128), (384, 768, 256)])
def test_gemm_q8_derivative(M, N, K, gemm_variant):
    """c2_mode 2 / A4R_DACT_MUL_Q8 (include/a4r.h): the saved GELU derivative as 8-bit fixed point.  The stored byte is the nearest
    level of gelu'(pre) (pre = the fp32 accumulator the kernel saw: a level off where bf16-rounded operands' fp32 sums differ in the
    last bits), the decoded value is within half a step, and the dgrad form multiplies by exactly the decoded value."""
    from adapter4rec_amd import _lib as L
    t = torch.bfloat16
    A, B = rnd(M, K, dtype=t, seed=3), rnd(N, K, dtype=t, scale=0.1, seed=4)
    bias = rnd(N, seed=5)
    Cc = torch.zeros(M, N, dtype=t, device=dev())
    C2 = torch.zeros(M, N, dtype=torch.uint8, device=dev())
    L.gemm_nt(A, B, Cc, bias=bias, C2=C2, act=L.ACT_GELU, c2_deriv='q8')
    pre = (A.float() @ B.float().t()) + bias
    q = pre.clone().requires_grad_(True)
    torch.nn.functional.gelu(q).sum().backward()
    close(Cc, torch.nn.functional.gelu(pre), t, 'gemm gelu (q8 second output)')
    dec = C2.float() * L.Q8_STEP - L.Q8_OFF
    err = (dec - q.grad).abs().max().item()
    assert err <= 0.5 * L.Q8_STEP + 2e-4, err
    lvl = torch.clamp(torch.round((q.grad + L.Q8_OFF) / L.Q8_STEP), 0, 255)
    assert (C2.float() - lvl).abs().max().item() <= 1 and (C2.float() != lvl).float().mean().item() < 0.01
    G = rnd(M, K, dtype=t, seed=9)                      # dgrad form: dX = (G W) * stored derivative, W [N, K]^T -> use B as [N_out, K]
    D = torch.zeros(M, N, dtype=t, device=dev())
    L.gemm_nt(G, B, D, Pre=C2, dact=L.DACT_MUL_Q8)
    close(D, (G.float() @ B.float().t()) * dec, t, 'gemm * q8 derivative')
    with pytest.raises(RuntimeError):                   # fp32 outputs have no 8-bit form
        L.gemm_nt(A.float(), B.float(), torch.zeros(M, N, device=dev()), C2=C2, act=L.ACT_GELU, c2_deriv='q8')
    with pytest.raises(RuntimeError):                   # GELU only
        L.gemm_nt(A, B, Cc, C2=C2, act=L.ACT_RELU, c2_deriv='q8')


@pytest.mark.parametrize('to', ['bf16', 'f32'])
def test_gemm_skinny64_epilogue(to):
    """N = 64 with bf16 operands goes to skinny64_kernel (a4r_gemm_skinny.hip): every epilogue form the adapter down-projections use
    (bias + ReLU/GELU + pre-activation or derivative in C2, residual, alpha, dropout) against torch and against the 128-tile kernel."""
    from adapter4rec_amd import _lib as L
    tO = DT[to]
    for M, K in ((128, 64), (384, 768), (4096 + 128, 320)):          # (the 128-tile comparison kernel needs M % 128 == 0)
        A, B = rnd(M, K, dtype=torch.bfloat16, seed=31), rnd(64, K, dtype=torch.bfloat16, scale=0.1, seed=32)
        bias, R1 = rnd(64, seed=33), rnd(M, 64, dtype=tO, seed=34)
        for act, c2d in ((1, 0), (1, 1), (2, 1), (0, 0)):
            outs = []
            for v in (2, 1):
                old = L.gemm_variant(v)
                Cc = torch.zeros(M, 64, dtype=tO, device=dev()); C2 = torch.zeros_like(Cc)
                L.gemm_nt(A, B, Cc, bias=bias, C2=C2, R1=R1, act=act, alpha=0.5, c2_deriv=bool(c2d))
                D = torch.zeros_like(Cc)
                L.gemm_nt(A, B, D, bias=bias, drop_p=0.2, drop_site=9, drop_seed=4321)
                L.gemm_variant(old)
                outs.append((Cc, C2, D))
            pre = 0.5 * (A.float() @ B.float().t()) + bias
            close(outs[0][0], act_ref(pre, act) + R1.float(), tO, f'skinny C act={act}')
            if c2d:
                q = pre.clone().requires_grad_(True)
                act_ref(q, act).sum().backward()
                close(outs[0][1], q.grad, tO, 'skinny C2 derivative')
            else:
                close(outs[0][1], pre, tO, 'skinny C2 pre-activation')
            close(outs[0][0], outs[1][0], tO, 'skinny vs 128-tile kernel', atol32=1e-5, rtol32=1e-5, atol16=1e-2, rtol16=1e-2)
            assert torch.equal(outs[0][2] == 0, outs[1][2] == 0), 'same dropout mask from both kernels'


def test_gemm_skinnyk_epilogue():
    """K = 64 (one K-tile) with bf16 operands goes to skinnyk_kernel (a4r_gemm_skinny.hip): bias, two residuals, alpha, ReLU, C2,
    dropout before / after the residual, in-place residual (C is R1); against torch and the 256-tile kernel (variant 4)."""
    from adapter4rec_amd import _lib as L
    t = torch.bfloat16
    for M, N in ((256, 256), (1024 + 256, 768), (512, 3072)):
        A, B = rnd(M, 64, dtype=t, seed=41), rnd(N, 64, dtype=t, scale=0.1, seed=42)
        bias, R1, R2 = rnd(N, seed=43), rnd(M, N, dtype=t, seed=44), rnd(M, N, dtype=t, seed=45)
        outs = []
        for v in (2, 4):
            old = L.gemm_variant(v)
            Cc = torch.zeros(M, N, dtype=t, device=dev()); C2 = torch.zeros_like(Cc)
            L.gemm_nt(A, B, Cc, bias=bias, C2=C2, R1=R1, R2=R2, act=1, alpha=0.5)
            D = torch.zeros_like(Cc)
            L.gemm_nt(A, B, D, bias=bias, R1=R1, drop_p=0.2, drop_site=9, drop_seed=4321, drop_first=True)
            E = R1.clone()
            L.gemm_nt(A, B, E, bias=bias, R1=E, R2=R2)                       # in place over R1
            L.gemm_variant(old)
            outs.append((Cc, C2, D, E))
        pre = 0.5 * (A.float() @ B.float().t()) + bias
        close(outs[0][0], torch.relu(pre) + R1.float() + R2.float(), t, 'skinnyk C')
        close(outs[0][1], pre, t, 'skinnyk C2')
        close(outs[0][3], (A.float() @ B.float().t()) + bias + R1.float() + R2.float(), t, 'skinnyk in place')
        for a, b in zip(outs[0], outs[1]):
            assert torch.equal(a, b), 'same MFMA order and epilogue as the 256-tile kernel: bit-equal'


def test_gemm_mixed_dtypes_and_views():
    from adapter4rec_amd import _lib as L
    M, N, K = 128, 64, 768
    big = rnd(M, K + 64, dtype=torch.bfloat16, seed=9)
    A = big[:, 64:]                          # lda != K
    B = rnd(N, K, dtype=torch.bfloat16, scale=0.05, seed=10)
    Cc = torch.zeros(M, N, dtype=torch.float32, device=dev())
    L.gemm_nt(A, B, Cc)
    close(Cc, A.float() @ B.float().t(), torch.float32, 'bf16->f32', atol32=2e-3, rtol32=1e-3)
    A32, B32 = rnd(M, 64, seed=11), rnd(768, 64, scale=0.1, seed=12)
    C16 = torch.zeros(M, 768, dtype=torch.bfloat16, device=dev())
    L.gemm_nt(A32, B32, C16)
    close(C16, A32 @ B32.t(), torch.bfloat16, 'f32->bf16')


def test_gemm_dropout_properties(gemm_variant):
    from adapter4rec_amd import _lib as L
    M, N, K = 256, 768, 128
    A, B = rnd(M, K, seed=13), rnd(N, K, seed=14)
    base = torch.zeros(M, N, device=dev())
    L.gemm_nt(A, B, base)
    d1, d2, d3 = torch.zeros_like(base), torch.zeros_like(base), torch.zeros_like(base)
    L.gemm_nt(A, B, d1, drop_p=0.1, drop_site=3, drop_seed=1234)
    L.gemm_nt(A, B, d2, drop_p=0.1, drop_site=3, drop_seed=1234)
    L.gemm_nt(A, B, d3, drop_p=0.1, drop_site=4, drop_seed=1234)
    assert torch.equal(d1, d2), 'dropout must be a pure function of (seed, site, index)'
    assert not torch.equal(d1, d3)
    kept = d1 != 0
    frac = 1.0 - kept.float().mean().item()
    assert abs(frac - 0.1) < 0.01, frac
    scale = 1.0 / (1.0 - round(0.1 * 65536) / 65536)
    torch.testing.assert_close(d1[kept], base[kept] * scale, rtol=1e-5, atol=1e-5)
    # forward form: dropout BEFORE the residual add (dense -> dropout -> + input)
    R = rnd(M, N, seed=15)
    d4 = torch.zeros_like(base)
    L.gemm_nt(A, B, d4, R1=R, drop_p=0.1, drop_site=3, drop_seed=1234, drop_first=True)
    torch.testing.assert_close(d4, d1 + R, rtol=1e-5, atol=1e-5)


def test_gemm_rejects_bad_shapes():
    from adapter4rec_amd import _lib as L
    A, B = rnd(100, 64), rnd(64, 64)
    with pytest.raises(RuntimeError):
        L.gemm_nt(A, B, torch.zeros(100, 64, device=dev()))      # M % 128 != 0


# ------------------------------------------------------------------ GEMM TN / colsum
@pytest.mark.parametrize('dt', ['f32', 'bf16'])
@pytest.mark.parametrize('M,P,Q', [(64, 64, 64), (1280, 768, 64), (1280, 64, 768), (640, 128, 192)])
def test_gemm_tn(dt, M, P, Q):
    from adapter4rec_amd import _lib as L
    t = DT[dt]
    X, Y = rnd(M, P, dtype=t, seed=15), rnd(M, Q, dtype=t, seed=16)
    Cc = torch.ones(P, Q, device=dev())
    L.gemm_tn(X, Y, Cc)
    ref = 1.0 + X.float().t() @ Y.float()
    close(Cc, ref, torch.float32, f'gemm_tn {dt}', atol32=2e-3 if dt == 'f32' else 2e-2, rtol32=1e-3)


@pytest.mark.parametrize('M,P,Q', [(40448, 768, 64), (40448, 64, 768), (64 * 37, 128, 192), (64, 64, 64), (128, 64, 64)])
def test_gemm_tn_glds_bf16(M, P, Q):
    """bf16 weight-gradient kernel (LDS-DMA ring + ds_read_b64_tr_b16): many splits, ragged last split, 1 and 2 stages; small-integer
    operands make the token sum exact, so it must equal torch AND the register-staged kernel bit for bit, views (ld > width) included."""
    from adapter4rec_amd import _lib as L
    g = torch.Generator().manual_seed(17)
    Xb = torch.randint(-3, 4, (M, P + 64), generator=g).to(torch.bfloat16).to(dev())
    Yb = torch.randint(-2, 3, (M, Q + 128), generator=g).to(torch.bfloat16).to(dev())
    X, Y = Xb[:, 64:], Yb[:, :Q]
    outs = []
    for v in (2, 0):
        old = L.gemm_variant(v)
        Cc = torch.full((P, Q), 3.0, device=dev())
        L.gemm_tn(X, Y, Cc)
        L.gemm_variant(old)
        outs.append(Cc)
    ref = 3.0 + X.float().t() @ Y.float()
    assert torch.equal(outs[0], ref), float((outs[0] - ref).abs().max())
    assert torch.equal(outs[0], outs[1])


@pytest.mark.parametrize('M,P,Q', [(40448, 768, 768), (40448, 3072, 768), (40448, 768, 3072), (4096, 256, 256), (64 * 67, 512, 256), (66304, 768, 2304)])
def test_gemm_tn_256_bf16(M, P, Q):
    """256 x 256-tile weight-gradient kernel (a4r_gemm_tn256.hip: trainable backbone Linears, --fine_tune_to all / Pretraining): token splits with a
    ragged last split, operands as views (ld > width: a slice of the fused qkv gradient), accumulation onto a non-zero C, and the column sums of
    X from the same launch (a4r_gemm_tn_bias).  Small-integer operands make every token sum exact in fp32 whatever the atomic order, so the
    result must equal torch AND the 64-tile kernel bit for bit."""
    from adapter4rec_amd import _lib as L
    g = torch.Generator().manual_seed(23)
    Xb = torch.randint(-3, 4, (M, P + 256), generator=g).to(torch.bfloat16).to(dev())
    Yb = torch.randint(-2, 3, (M, Q + 64), generator=g).to(torch.bfloat16).to(dev())
    X, Y = Xb[:, 256:], Yb[:, :Q]
    ref = 3.0 + X.float().t() @ Y.float()
    Cc = torch.full((P, Q), 3.0, device=dev())
    L.gemm_tn(X, Y, Cc)
    assert torch.equal(Cc, ref), float((Cc - ref).abs().max())
    old = L.gemm_variant(0)                                   # the register-staged 64-tile kernel
    C0 = torch.full((P, Q), 3.0, device=dev())
    L.gemm_tn(X, Y, C0)
    L.gemm_variant(old)
    assert torch.equal(C0, ref)
    Cb, xs = torch.full((P + 64, Q + 64), 3.0, device=dev()), torch.full((P,), -2.0, device=dev())
    L.gemm_tn_bias(X, Y, Cb[:P, :Q], xs)                      # C as a view too
    assert torch.equal(Cb[:P, :Q], ref)
    assert torch.equal(Cb[P:], torch.full_like(Cb[P:], 3.0)) and torch.equal(Cb[:, Q:], torch.full_like(Cb[:, Q:], 3.0))
    assert torch.equal(xs, -2.0 + X.float().sum(0)), float((xs + 2.0 - X.float().sum(0)).abs().max())


@pytest.mark.parametrize('M,H,n', [(40448, 768, 4), (4096, 256, 2), (64 * 67, 512, 3), (1280, 64, 4)])
def test_gemm_tn_multi(M, H, n):
    """a4r_gemm_tn_multi: the q / k / v weight + bias gradients (X = column slices of one fused [M, 3H] gradient, Y = the shared block input) and the
    attention output's (its own operands) over the same token rows in ONE call -- one launch of the 256-tile kernel when H % 256 == 0, the
    per-product path otherwise (H = 64).  Exact small-integer operands: equal to torch bit for bit; a product without xsum leaves nothing behind."""
    from adapter4rec_amd import _lib as L
    g = torch.Generator().manual_seed(29)
    dqkv = torch.randint(-3, 4, (M, 3 * H), generator=g).to(torch.bfloat16).to(dev())
    xin = torch.randint(-2, 3, (M, H), generator=g).to(torch.bfloat16).to(dev())
    dh1 = torch.randint(-2, 3, (M, H), generator=g).to(torch.bfloat16).to(dev())
    ctx = torch.randint(-3, 4, (M, H + 64), generator=g).to(torch.bfloat16).to(dev())[:, 64:]
    ops = [(dqkv[:, i * H:(i + 1) * H], xin) for i in range(3)] + [(dh1, ctx)]
    ops = ops[4 - n:]
    Cs = [torch.full((H, H), float(i), device=dev()) for i in range(n)]
    xs = [None if i == 1 else torch.full((H,), 0.5 * i, device=dev()) for i in range(n)]
    L.gemm_tn_multi([(X, Y, Cc, x) for (X, Y), Cc, x in zip(ops, Cs, xs)])
    for i, ((X, Y), Cc, x) in enumerate(zip(ops, Cs, xs)):
        ref = float(i) + X.float().t() @ Y.float()
        assert torch.equal(Cc, ref), (i, float((Cc - ref).abs().max()))
        if x is not None:
            assert torch.equal(x, 0.5 * i + X.float().sum(0)), i
    with pytest.raises(RuntimeError):
        L.gemm_tn_multi([(ops[0][0], ops[0][1], Cs[0], None)] * 5 if False else [(ops[0][0][:, :32], ops[0][1], Cs[0][:32], None)])      # P % 64 != 0


def test_gemm_tn_bias_small_shapes_fall_back():
    """a4r_gemm_tn_bias on shapes the 256-tile kernel does not take (adapter-sized outputs, fp32): a4r_gemm_tn + a4r_colsum."""
    from adapter4rec_amd import _lib as L
    for t, M, P, Q in ((torch.bfloat16, 1280, 768, 64), (torch.float32, 640, 64, 128), (torch.bfloat16, 2048, 256, 256)):
        X, Y = rnd(M, P, dtype=t, seed=61), rnd(M, Q, dtype=t, seed=62)
        Cc, xs = torch.zeros(P, Q, device=dev()), torch.zeros(P, device=dev())
        L.gemm_tn_bias(X, Y, Cc, xs)
        close(Cc, X.float().t() @ Y.float(), torch.float32, 'tn_bias C', atol32=2e-2, rtol32=2e-3)
        close(xs, X.float().sum(0), torch.float32, 'tn_bias xsum', atol32=2e-2, rtol32=2e-3)


def test_gemm_tn2_two_products_one_launch():
    """a4r_gemm_tn2 = two a4r_gemm_tn products over the same rows (an adapter's dW_up [H, 64] and dW_down [64, H])."""
    from adapter4rec_amd import _lib as L
    t = torch.bfloat16
    for M, H in ((1280, 768), (4096, 128), (192, 256)):
        X1, Y1 = rnd(M, H, dtype=t, seed=51), rnd(M, 64, dtype=t, seed=52)
        X2, Y2 = rnd(M, 64, dtype=t, seed=53), rnd(M, H, dtype=t, seed=54)
        C1, C2 = torch.zeros(H, 64, device=dev()), torch.zeros(64, H, device=dev())
        L.gemm_tn2(X1, Y1, C1, X2, Y2, C2)
        close(C1, X1.float().t() @ Y1.float(), torch.float32, 'tn2 first', atol32=2e-3 * (M / 1280) ** 0.5 * 8, rtol32=2e-3)
        close(C2, X2.float().t() @ Y2.float(), torch.float32, 'tn2 second', atol32=2e-3 * (M / 1280) ** 0.5 * 8, rtol32=2e-3)
        # + the column sums of both X operands from the same pass (the bias gradients that go with the two weight gradients), accumulating
        C1b, C2b = torch.zeros_like(C1), torch.zeros_like(C2)
        s1, s2 = torch.full((H,), 0.5, device=dev()), torch.full((64,), -1.0, device=dev())
        L.gemm_tn2(X1, Y1, C1b, X2, Y2, C2b, xsum1=s1, xsum2=s2)
        assert torch.equal(C1b, C1) or float((C1b - C1).abs().max()) < 1e-3           # (atomic order differs between launches)
        close(s1, 0.5 + X1.float().sum(0), torch.float32, 'tn2 xsum1', atol32=2e-3 * (M / 1280) ** 0.5 * 8, rtol32=2e-3)
        close(s2, -1.0 + X2.float().sum(0), torch.float32, 'tn2 xsum2', atol32=2e-3 * (M / 1280) ** 0.5 * 8, rtol32=2e-3)
        s3 = torch.zeros(H, device=dev())
        L.gemm_tn2(X1, Y1, C1b, X2, Y2, C2b, xsum1=s3)                                    # one of the two only
        close(s3, X1.float().sum(0), torch.float32, 'tn2 xsum1 alone', atol32=2e-3 * (M / 1280) ** 0.5 * 8, rtol32=2e-3)
    with pytest.raises(RuntimeError):                                          # unequal tile counts
        L.gemm_tn2(X1, Y1, C1, X2, rnd(192, 128, dtype=t, seed=55), torch.zeros(64, 128, device=dev()))


@pytest.mark.parametrize('dt', ['f32', 'bf16'])
def test_colsum(dt):
    from adapter4rec_amd import _lib as L
    t = DT[dt]
    for M, N in [(1280, 768), (640, 64), (100, 16), (66304, 768), (40448, 64), (7, 8)]:
        X = rnd(M, N, dtype=t, seed=17)
        out = torch.zeros(N, device=dev())
        L.colsum(X, out)
        close(out, X.float().sum(0), torch.float32, 'colsum', atol32=2e-3 * max(1.0, (M / 1280) ** 0.5), rtol32=1e-3)


# ------------------------------------------------------------------ attention
def attn_ref(qkv, key_mask, n_items, S, nh, dh, causal, scale, mask_neg, offs):
    Hd = nh * dh
    q, k, v = [qkv[:n_items * S, o:o + Hd].float().view(n_items, S, nh, dh).transpose(1, 2) for o in offs]
    sc = q @ k.transpose(-1, -2) * scale
    allowed = (key_mask != 0)[:, None, None, :].expand(n_items, 1, S, S)
    if causal:
        allowed = torch.tril(allowed)
    sc = sc + torch.where(allowed, torch.zeros((), device=sc.device), torch.full((), mask_neg, device=sc.device))
    p = torch.softmax(sc, -1)
    return (p @ v).transpose(1, 2).reshape(n_items * S, Hd)


ATTN_CASES = [('bert', 30, 12, 64, False, torch.finfo(torch.float32).min), ('bert2', 30, 2, 64, False, torch.finfo(torch.float32).min),
              ('sasrec', 20, 2, 32, True, -1e9), ('full32', 32, 3, 64, True, -1e9),
              ('kad_bert', 30, 12, 16, False, -10000.0), ('kad_sas', 20, 2, 8, True, -1e9), ('kad_odd', 7, 3, 8, False, -1e9)]


@pytest.mark.parametrize('dt', ['f32', 'bf16'])
@pytest.mark.parametrize('name,S,nh,dh,causal,neg', ATTN_CASES)
def test_attention_fwd_bwd(dt, name, S, nh, dh, causal, neg):
    from adapter4rec_amd import _lib as L
    t = DT[dt]
    n_items, Hd = 11, nh * dh
    Mp = ((n_items * S + 127) // 128) * 128
    qkv = rnd(Mp, 3 * Hd, dtype=t, seed=21)
    km = torch.ones(n_items, S)
    km[1, S // 2:] = 0                    # ragged title
    km[2, :] = 0                          # all-PAD item: fully masked rows must stay finite (uniform softmax)
    km[3, :3] = 0                         # left padding (SASRec style)
    km = km.to(dev())
    scale = 1.0 / math.sqrt(dh)
    offs = (0, Hd, 2 * Hd)
    out = torch.zeros(Mp, Hd, dtype=t, device=dev())
    L.attn_fwd(qkv, out, km, n_items, S, nh, dh, *offs, causal, scale, neg)
    qr = qkv.float().clone().requires_grad_(True)
    ref = attn_ref(qr, km, n_items, S, nh, dh, causal, scale, neg, offs)
    close(out[:n_items * S], ref.detach(), t, f'attn fwd {name} {dt}', atol32=1e-4, rtol32=1e-4)
    assert torch.count_nonzero(out[n_items * S:]) == 0
    dout = rnd(Mp, Hd, dtype=t, seed=22)
    dout[n_items * S:] = 0
    dqkv = torch.zeros_like(qkv)
    L.attn_bwd(qkv, dout, dqkv, km, n_items, S, nh, dh, *offs, causal, scale, neg)
    ref.backward(dout[:n_items * S].float())
    close(dqkv[:n_items * S], qr.grad[:n_items * S], t, f'attn bwd {name} {dt}', atol32=2e-4, rtol32=2e-4,
          atol16=4e-2 * float(qr.grad.abs().max()))


LONG_CASES = [('f32', 33, 2, 64), ('f32', 50, 12, 64), ('f32', 64, 3, 64), ('f32', 100, 2, 64), ('f32', 128, 2, 64),
              ('f32', 197, 12, 64), ('f32', 256, 2, 64),      # round 3: the fp32 backward fits ViT-B/16's S = 197 (no transposed LDS copies)
              ('bf16', 33, 2, 64), ('bf16', 50, 12, 64), ('bf16', 65, 3, 64), ('bf16', 128, 2, 64), ('bf16', 197, 12, 64),
              ('bf16', 224, 2, 64), ('bf16', 256, 2, 64),
              # head width 32: the K-Adapter blocks of VITKAdaptedCVModel (width 384, 12 heads; S = 197 / 50)
              ('f32', 33, 2, 32), ('f32', 50, 12, 32), ('f32', 100, 3, 32), ('f32', 197, 12, 32), ('f32', 256, 2, 32),
              ('bf16', 40, 2, 32), ('bf16', 50, 12, 32), ('bf16', 128, 3, 32), ('bf16', 197, 12, 32), ('bf16', 256, 2, 32)]


@pytest.mark.parametrize('dt,S,nh,dh', LONG_CASES)
def test_attention_long_fwd_bwd(dt, S, nh, dh):
    """a4r_attn_long_*: the un-masked ViT / MAE attention (S up to 256, dh 64 / 32) against fp32 torch softmax(QK^T/sqrt(dh))V."""
    from adapter4rec_amd import _lib as L
    t = DT[dt]
    n_items = 5
    Hd = nh * dh
    Mp = ((n_items * S + 255) // 256) * 256
    qkv = rnd(Mp, 3 * Hd, dtype=t, seed=31 + S)
    scale = 1.0 / math.sqrt(dh)
    offs = (0, Hd, 2 * Hd)
    out = torch.zeros(Mp, Hd, dtype=t, device=dev())
    lse = torch.zeros(n_items * nh * S, device=dev())
    L.attn_long_fwd(qkv, out, lse, n_items, S, nh, dh, *offs, scale)
    qr = qkv.float().clone().requires_grad_(True)
    ref = attn_ref(qr, torch.ones(n_items, S, device=dev()), n_items, S, nh, dh, False, scale, 0.0, offs)
    close(out[:n_items * S], ref.detach(), t, f'attn_long fwd S={S} {dt}', atol32=1e-4, rtol32=1e-4)
    assert torch.count_nonzero(out[n_items * S:]) == 0
    q, k = [qkv[:n_items * S, o:o + Hd].float().view(n_items, S, nh, dh).transpose(1, 2) for o in offs[:2]]
    lse_ref = torch.logsumexp(q @ k.transpose(-1, -2) * scale, -1).reshape(-1)
    close(lse, lse_ref, torch.float32, 'lse', atol32=1e-3 if t == torch.float32 else 2e-2, rtol32=1e-3)
    dout = rnd(Mp, Hd, dtype=t, seed=32)
    dout[n_items * S:] = 0
    dqkv = torch.zeros_like(qkv)
    ws = torch.zeros_like(lse)
    L.attn_long_bwd(qkv, out, dout, dqkv, lse, ws, n_items, S, nh, dh, *offs, scale)
    ref.backward(dout[:n_items * S].float())
    close(dqkv[:n_items * S], qr.grad[:n_items * S], t, f'attn_long bwd S={S} {dt}', atol32=2e-4, rtol32=2e-4,
          atol16=4e-2 * float(qr.grad.abs().max()))
    assert torch.count_nonzero(dqkv[n_items * S:]) == 0


@pytest.mark.parametrize('dt,S,nh', [('f32', 33, 2), ('f32', 50, 12), ('f32', 100, 3), ('f32', 197, 2), ('f32', 256, 2),
                                     ('bf16', 40, 2), ('bf16', 50, 12), ('bf16', 64, 4), ('bf16', 128, 3), ('bf16', 197, 2), ('bf16', 256, 2)])
def test_attention_long_key_mask_fwd_bwd(dt, S, nh):
    """a4r_attn_long_* WITH a key mask (round 5: text towers with --num_words_title > 32; head width 64): prefix masks of different lengths, a mask with
    holes, a full one and an item without any attended key (the PAD item: uniform attention over its S keys, as HF's softmax over S equal scores),
    forward, lse and backward against fp32 torch softmax(QK^T / sqrt(dh) + (1 - mask) finfo.min) V."""
    from adapter4rec_amd import _lib as L
    t, dh = DT[dt], 64
    n_items = 6
    Hd = nh * dh
    Mp = ((n_items * S + 255) // 256) * 256
    qkv = rnd(Mp, 3 * Hd, dtype=t, seed=131 + S)
    scale = 1.0 / math.sqrt(dh)
    offs = (0, Hd, 2 * Hd)
    km = torch.zeros(n_items, S, device=dev())
    km[0, :S] = 1
    km[1, :4] = 1
    km[2, :S // 2 + 3] = 1
    km[3, ::3] = 1                                    # holes
    km[4, :1] = 1                                     # [CLS] only
    # item 5: nothing attended
    out = torch.zeros(Mp, Hd, dtype=t, device=dev())
    lse = torch.zeros(n_items * nh * S, device=dev())
    L.attn_long_fwd(qkv, out, lse, n_items, S, nh, dh, *offs, scale, key_mask=km)
    qr = qkv.float().clone().requires_grad_(True)
    FMIN = torch.finfo(torch.float32).min
    ref = attn_ref(qr, km, n_items, S, nh, dh, False, scale, FMIN, offs)
    close(out[:n_items * S], ref.detach(), t, f'attn_long masked fwd S={S} {dt}', atol32=1e-4, rtol32=1e-4)
    dout = rnd(Mp, Hd, dtype=t, seed=132)
    dout[n_items * S:] = 0
    dqkv = torch.zeros_like(qkv)
    ws = torch.zeros_like(lse)
    L.attn_long_bwd(qkv, out, dout, dqkv, lse, ws, n_items, S, nh, dh, *offs, scale, key_mask=km)
    ref.backward(dout[:n_items * S].float())
    assert torch.isfinite(dqkv.float()).all()
    close(dqkv[:n_items * S], qr.grad[:n_items * S], t, f'attn_long masked bwd S={S} {dt}', atol32=2e-4, rtol32=2e-4,
          atol16=4e-2 * float(qr.grad.abs().max()))
    # a masked key receives no gradient through K / V (item 1: keys >= 4)
    assert float(dqkv[S + 4:2 * S, Hd:].float().abs().max()) == 0.0


@pytest.mark.parametrize('dt,S,nh,dh,all_rows', [('f32', 40, 2, 32, False), ('f32', 50, 2, 32, False), ('f32', 100, 2, 64, False), ('f32', 200, 2, 32, False),
                                                 ('bf16', 50, 2, 32, False), ('bf16', 64, 4, 64, False), ('bf16', 130, 2, 32, False), ('f32', 20, 2, 32, False),
                                                 ('f32', 40, 2, 32, True), ('f32', 100, 2, 64, True), ('bf16', 50, 2, 32, True),
                                                 ('f32', 40, 2, 128, False), ('f32', 100, 2, 128, True), ('f32', 128, 1, 128, False), ('f32', 24, 2, 128, False)])
def test_attention_long_causal_key_mask_fwd_bwd(dt, S, nh, dh, all_rows):
    """a4r_attn_long_* causal + key mask (round 5: the user tower at --max_seq_len > 32; SelfAttention of model/modules.py:31-42 with the mask of
    model/encoders.py:24-28 = log_mask AND lower-triangular, -1e9 added elsewhere): left-padded histories of different lengths (their padded
    positions are queries without any allowed key: uniform attention, no gradient), a full one, an empty one; forward and backward against fp32 torch."""
    from adapter4rec_amd import _lib as L
    t = DT[dt]
    n_items = 5
    Hd = nh * dh
    Mp = ((n_items * S + 255) // 256) * 256
    qkv = rnd(Mp, 3 * Hd, dtype=t, seed=231 + S)
    scale = 1.0 / math.sqrt(dh)
    offs = (0, Hd, 2 * Hd)
    km = torch.zeros(n_items, S, device=dev())
    km[0, :] = 1
    km[1, S - 3:] = 1                                  # a short history: positions 0 .. S-4 are padding
    km[2, S // 2:] = 1
    km[3, 1:] = 1
    # item 4: nothing attended
    out = torch.zeros(Mp, Hd, dtype=t, device=dev())
    lse = torch.zeros(n_items * nh * S, device=dev())
    L.attn_long_fwd(qkv, out, lse, n_items, S, nh, dh, *offs, scale, key_mask=km, causal=True)
    qr = qkv.float().clone().requires_grad_(True)
    ref = attn_ref(qr, km, n_items, S, nh, dh, True, scale, -1e9, offs)
    close(out[:n_items * S], ref.detach(), t, f'attn_long causal fwd S={S} {dt}', atol32=1e-4, rtol32=1e-4)
    dout = rnd(Mp, Hd, dtype=t, seed=232)
    dout[n_items * S:] = 0
    allowed_any = (torch.tril(torch.ones(S, S, device=dev()))[None] * km[:, None, :]).sum(-1) > 0          # [item, query]
    if not all_rows:                                    # rows behind the loss mask carry no gradient in the model; all_rows: they do here -- the kernels then apply
        dout[:n_items * S] = dout[:n_items * S] * allowed_any.reshape(-1, 1).to(t)      # the Jacobian of the uniform row over all S keys, as autograd does
    dqkv = torch.zeros_like(qkv)
    ws = torch.zeros_like(lse)
    L.attn_long_bwd(qkv, out, dout, dqkv, lse, ws, n_items, S, nh, dh, *offs, scale, key_mask=km, causal=True)
    ref.backward(dout[:n_items * S].float())
    assert torch.isfinite(dqkv.float()).all()
    close(dqkv[:n_items * S], qr.grad[:n_items * S], t, f'attn_long causal bwd S={S} {dt}', atol32=2e-4, rtol32=2e-4,
          atol16=4e-2 * float(qr.grad.abs().max()))


@pytest.mark.parametrize('form', ['0', '1'])
def test_attention_long_backward_both_launch_forms(form):
    """A4R_ATTN_BWD_FUSED=0 / 1 force the two-launch / one-launch backward for EVERY sequence length (the default picks by length; the switch is read
    once per process, hence the child process): the un-masked, key-masked and causal backward tests must pass in both forms."""
    import os
    import subprocess
    import sys
    env = dict(os.environ, A4R_ATTN_BWD_FUSED=form, A4R_ATTN_BWD_ONEPASS='0')      # (the persistent one-pass kernel, the default at 129 .. 224 tokens, would take ViT-B/16's shape from both)
    r = subprocess.run([sys.executable, '-m', 'pytest', os.path.abspath(__file__), '-q', '-x', '-p', 'no:cacheprovider',
                        '-k', 'attention_long_fwd_bwd or attention_long_key_mask or attention_long_causal or attention_long_dropout'],
                       env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert ' passed' in r.stdout and 'failed' not in r.stdout, r.stdout[-500:]


def test_attention_long_rejects():
    from adapter4rec_amd import _lib as L
    qkv = torch.zeros(512, 192, device=dev())
    out = torch.zeros(512, 64, device=dev())
    lse = torch.zeros(512, device=dev())
    # (round 3: the fp32 backward at S = 200 no longer raises -- it reads its transposed operands from the row-major LDS images and
    # fits; test_attention_long_fp32_s197 below checks it against autograd)
    with pytest.raises(RuntimeError):
        L.attn_long_fwd(qkv, out, lse, 1, 300, 1, 64, 0, 64, 128, 0.125)       # S > 256
    with pytest.raises(RuntimeError):
        L.attn_long_fwd(qkv, out, lse, 1, 100, 1, 48, 0, 64, 128, 0.125)       # head width other than 64 / 32
    q2, o2 = torch.zeros(512, 384, device=dev()), torch.zeros(512, 128, device=dev())
    with pytest.raises(RuntimeError):
        L.attn_long_fwd(q2, o2, lse, 1, 200, 1, 128, 0, 128, 256, 0.1)           # head width 128: up to 128 tokens
    with pytest.raises(RuntimeError):
        L.attn_long_fwd(q2.bfloat16(), o2.bfloat16(), lse, 1, 100, 1, 128, 0, 128, 256, 0.1)      # ... and fp32 only
    with pytest.raises(RuntimeError):
        L.attn_long_fwd(qkv, out, lse, 1, 100, 1, 64, 0, 64, 128, 0.125, drop_p=1.0)


@pytest.mark.parametrize('dt,S,nh,dh', [('f32', 64, 2, 64), ('f32', 100, 3, 32), ('bf16', 197, 12, 32), ('bf16', 197, 2, 64), ('bf16', 50, 12, 32)])
def test_attention_long_dropout(dt, S, nh, dh):
    """Dropout on the probabilities (SelfAttention.dropout, CV modules.py:35) in the long kernels.  The mask is read back from the
    forward kernel itself (Q = K = 0 makes P uniform, V = a shifted identity exposes P' column block by column block; the mask is
    a function of (seed, site, item, head, query, key) only), then forward and all three gradients are held to torch autograd
    with that mask: forward, dq and dk/dv launches must regenerate exactly the same keep pattern."""
    from adapter4rec_amd import _lib as L
    t = DT[dt]
    n_items, p, site, seed = 3, 0.3, 11, 1234
    Hd = nh * dh
    Mp = ((n_items * S + 255) // 256) * 256
    offs = (0, Hd, 2 * Hd)
    scale = 1.0 / math.sqrt(dh)
    lse = torch.zeros(n_items * nh * S, device=dev())
    keep = torch.zeros(n_items, nh, S, S, device=dev())
    for blk in range((S + dh - 1) // dh):
        probe = torch.zeros(Mp, 3 * Hd, dtype=t, device=dev())
        v = probe[:n_items * S, 2 * Hd:].view(n_items, S, nh, dh)
        for j in range(min(dh, S - blk * dh)):
            v[:, blk * dh + j, :, j] = 1.0
        o = torch.zeros(Mp, Hd, dtype=t, device=dev())
        L.attn_long_fwd(probe, o, lse, n_items, S, nh, dh, *offs, scale, drop_p=p, drop_site=site, drop_seed=seed)
        blkv = o[:n_items * S].float().view(n_items, S, nh, dh).permute(0, 2, 1, 3)[..., :min(dh, S - blk * dh)]
        keep[..., blk * dh:blk * dh + blkv.shape[-1]] = (blkv > 0).float()
    frac = keep.mean().item()
    assert abs(frac - (1 - p)) < 0.01, frac
    ks = 1.0 / (1.0 - round(p * 65536) / 65536.0)
    qkv = rnd(Mp, 3 * Hd, dtype=t, seed=41 + S)
    out = torch.zeros(Mp, Hd, dtype=t, device=dev())
    L.attn_long_fwd(qkv, out, lse, n_items, S, nh, dh, *offs, scale, drop_p=p, drop_site=site, drop_seed=seed)
    qr = qkv.float().clone().requires_grad_(True)
    q, k, v = [qr[:n_items * S, o_:o_ + Hd].view(n_items, S, nh, dh).transpose(1, 2) for o_ in offs]
    pr = torch.softmax(q @ k.transpose(-1, -2) * scale, -1) * keep * ks
    ref = (pr @ v).transpose(1, 2).reshape(n_items * S, Hd)
    close(out[:n_items * S], ref.detach(), t, f'attn_long dropout fwd S={S} {dt}', atol32=1e-4, rtol32=1e-4)
    dout = rnd(Mp, Hd, dtype=t, seed=42)
    dout[n_items * S:] = 0
    dqkv = torch.zeros_like(qkv)
    L.attn_long_bwd(qkv, out, dout, dqkv, lse, torch.zeros_like(lse), n_items, S, nh, dh, *offs, scale, drop_p=p, drop_site=site, drop_seed=seed)
    ref.backward(dout[:n_items * S].float())
    close(dqkv[:n_items * S], qr.grad[:n_items * S], t, f'attn_long dropout bwd S={S} {dt}', atol32=2e-4, rtol32=2e-4,
          atol16=4e-2 * float(qr.grad.abs().max()))


@pytest.mark.parametrize('dt', ['f32', 'bf16'])
@pytest.mark.parametrize('dh', [64, 8])
def test_attention_dropout_adjoint(dt, dh):
    """With dropout on, out is linear in V: <out, dO> == <V, dV> iff fwd and bwd regenerate the same mask."""
    from adapter4rec_amd import _lib as L
    t = DT[dt]
    n_items, S, nh = 9, 30, 4
    Hd = nh * dh
    Mp = 384
    qkv = rnd(Mp, 3 * Hd, dtype=t, seed=23)
    km = torch.ones(n_items, S, device=dev())
    args = (km, n_items, S, nh, dh, 0, Hd, 2 * Hd, False, 0.125, -1e9)
    out = torch.zeros(Mp, Hd, dtype=t, device=dev())
    out0 = torch.zeros_like(out)
    L.attn_fwd(qkv, out0, *args)
    L.attn_fwd(qkv, out, *args, drop_p=0.25, drop_site=5, drop_seed=77)
    assert not torch.allclose(out.float(), out0.float())
    dout = rnd(Mp, Hd, dtype=t, seed=24)
    dout[n_items * S:] = 0
    dqkv = torch.zeros_like(qkv)
    L.attn_bwd(qkv, dout, dqkv, *args, drop_p=0.25, drop_site=5, drop_seed=77)
    lhs = (out.float() * dout.float()).sum().item()
    rhs = (qkv[:, 2 * Hd:].float() * dqkv[:, 2 * Hd:].float()).sum().item()
    assert abs(lhs - rhs) <= (2e-3 if dt == 'f32' else 3e-2) * max(1.0, abs(lhs)), (lhs, rhs)


# ------------------------------------------------------------------ row kernels
@pytest.mark.parametrize('dt', ['f32', 'bf16'])
@pytest.mark.parametrize('roberta', [False, True])
def test_embed_ln(dt, roberta):
    from adapter4rec_amd import _lib as L
    t = DT[dt]
    n_items, S, H, V = 7, 30, 768, 500
    g = torch.Generator().manual_seed(5)
    ids = torch.randint(3, V, (n_items, 2 * S), generator=g)
    pad = 1 if roberta else 0
    ids[1, 10:S] = pad
    ids[2, :S] = 0
    ids = ids.to(dev())
    word, pos, typ = rnd(V, H, seed=31), rnd(S + 4, H, seed=32), rnd(2, H, seed=33)
    gamma, beta = rnd(H, seed=34) * 0.1 + 1, rnd(H, seed=35) * 0.1
    out = torch.zeros(256, H, dtype=t, device=dev())
    L.embed_ln(ids, word, pos, typ[0].contiguous(), gamma, beta, 1e-12, out, n_items, S, roberta=roberta, pad_id=pad)
    idv = ids[:, :S]
    if roberta:
        m = (idv != pad).long()
        pid = torch.cumsum(m, 1) * m + pad
    else:
        pid = torch.arange(S, device=dev()).expand(n_items, S)
    x = word[idv] + pos[pid] + typ[0]
    ref = torch.nn.functional.layer_norm(x, (H,), gamma, beta, 1e-12).view(-1, H)
    close(out[:n_items * S], ref, t, f'embed_ln {dt}', atol32=1e-4)


@pytest.mark.parametrize('dt', ['f32', 'bf16'])
@pytest.mark.parametrize('H', [64, 128, 768, 1024])
def test_ln_fwd_bwd(dt, H):
    from adapter4rec_amd import _lib as L
    t = DT[dt]
    M = 256
    v = rnd(M, H, dtype=t, seed=41, scale=2.0)
    add = rnd(20, H, seed=42) if H == 64 else None
    gamma, beta = rnd(H, seed=43) * 0.2 + 1, rnd(H, seed=44) * 0.1
    y = torch.zeros(M, H, dtype=t, device=dev())
    stats = torch.zeros(M, 2, device=dev())
    L.ln_fwd(v, gamma, beta, 1e-6, y, stats, add=add)
    vr = v.float().clone().requires_grad_(True)
    gr, br = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    vin = vr + (add[torch.arange(M, device=dev()) % 20] if add is not None else 0)
    ref = torch.nn.functional.layer_norm(vin, (H,), gr, br, 1e-6)
    close(y, ref.detach(), t, f'ln fwd H={H}', atol32=1e-4)
    dy = rnd(M, H, dtype=t, seed=45)
    dv = torch.zeros(M, H, dtype=t, device=dev())
    dg, db, dbias = torch.zeros(H, device=dev()), torch.zeros(H, device=dev()), torch.zeros(H, device=dev())
    L.ln_bwd(dy, v, stats, gamma, dv, add=add, dgamma=dg, dbeta=db, dbias=dbias)
    ref.backward(dy.float())
    close(dv, vr.grad, t, f'ln bwd dv H={H}', atol32=2e-4)
    tol = dict(atol32=5e-3, rtol32=2e-3) if dt == 'f32' else dict(atol32=0.5, rtol32=5e-2)
    close(dg, gr.grad, torch.float32, 'ln dgamma', **tol)
    close(db, br.grad, torch.float32, 'ln dbeta', **tol)
    close(dbias, vr.grad.sum(0), torch.float32, 'ln dbias', **tol)   # summed in fp32 before dv is rounded


@pytest.mark.parametrize('dt', ['f32', 'bf16'])
@pytest.mark.parametrize('M,H', [(1, 768), (4 * 2048 + 3, 768), (777, 384), (130, 1024), (4 * 2048 * 3 + 17, 64)])
def test_ln_lean_forms_equal_general(dt, M, H):
    """The lean LayerNorm kernels (no additive table / dropout / e4m3 output; backward without parameter gradients or a second output: what the image
    tower's un-adapted sub-layers launch) against the general kernels on the same rows -- the general form is forced with an all-zero additive table --
    and against torch fp32: every row count around the grid-stride loop's edges (one row, a partial last round, more than two rounds), group counts
    that leave the second 8-element group of a lane empty (H = 384, 64), half full (768) and full (1024), with and without the residual-branch operand."""
    from adapter4rec_amd import _lib as L
    t = DT[dt]
    v, dy, dres = rnd(M, H, dtype=t, seed=71, scale=2.0), rnd(M, H, dtype=t, seed=72), rnd(M, H, dtype=t, seed=73)
    gamma, beta = rnd(H, seed=74) * 0.2 + 1, rnd(H, seed=75) * 0.1
    zero_add = torch.zeros(1, H, device=dev())
    y_l, y_g = torch.zeros(M, H, dtype=t, device=dev()), torch.zeros(M, H, dtype=t, device=dev())
    st_l, st_g = torch.zeros(M, 2, device=dev()), torch.zeros(M, 2, device=dev())
    L.ln_fwd(v, gamma, beta, 1e-6, y_l, st_l)
    L.ln_fwd(v, gamma, beta, 1e-6, y_g, st_g, add=zero_add)
    assert torch.equal(y_l, y_g) and torch.equal(st_l, st_g)
    ref = torch.nn.functional.layer_norm(v.float(), (H,), gamma, beta, 1e-6)
    close(y_l, ref, t, f'lean ln fwd M={M} H={H}', atol32=1e-4)
    for res in (None, dres):
        dv_l, dv_g = torch.zeros(M, H, dtype=t, device=dev()), torch.zeros(M, H, dtype=t, device=dev())
        L.ln_bwd(dy, v, st_l, gamma, dv_l, dres=res)
        L.ln_bwd(dy, v, st_l, gamma, dv_g, dres=res, add=zero_add)
        if dt == 'f32':
            torch.testing.assert_close(dv_l, dv_g, rtol=1e-5, atol=1e-5)        # same arithmetic, xhat rebuilt in the second pass
        else:
            torch.testing.assert_close(dv_l.float(), dv_g.float(), rtol=2 ** -7, atol=2 ** -7)
        vr = v.float().clone().requires_grad_(True)
        torch.nn.functional.layer_norm(vr, (H,), gamma, beta, 1e-6).backward(dy.float())
        want = vr.grad + (res.float() if res is not None else 0)
        close(dv_l, want, t, f'lean ln bwd M={M} H={H}', atol32=3e-4)


@pytest.mark.parametrize('R,ra,rb', [(8, 8, 5), (16, 12, 12), (16, 15, 9)])
@pytest.mark.parametrize('M,bias', [(16, True), (16 * 257, True), (16 * 1200 + 16, False)])
def test_lora_bwd_fused(M, bias, R, ra, rb):
    """a4r_lora_bwd_fused against its CPU restatement (tests/sim_lib.py, pinned to the five products it replaces by tests/test_lora_fused_cpu.py): one
    tile, one tile per workgroup + 1, many tiles per workgroup; both rank-tile forms (ranks <= 8 share a tile; 9 - 15, the image tower's hard-coded
    12, get one each); strided operands and outputs as the engine hands them over (slices of the fused qkv gradient, rank rows 0 .. / 16 .. of 64-row
    weight operands, corners of the fp32 scratch matrices, the bias sums in a column of one of them); outputs are ACCUMULATED into."""
    from adapter4rec_amd import _lib as L
    import sim_lib as S
    H, rp, oc, T = 768, 64, 32, torch.bfloat16
    x = rnd(M, H, dtype=T, seed=81)
    dqkv = rnd(M, 3 * H, dtype=T, seed=82, scale=0.1)
    dqa, dqb = dqkv[:, :H], dqkv[:, 2 * H:]
    A, BTa, BTb = (torch.zeros(rp, H, dtype=T, device=dev()) for _ in range(3))
    A[0:ra], A[16:16 + rb] = rnd(ra, H, dtype=T, seed=83, scale=0.05), rnd(rb, H, dtype=T, seed=84, scale=0.05)
    BTa[0:ra], BTb[16:16 + rb] = rnd(ra, H, dtype=T, seed=85, scale=0.05), rnd(rb, H, dtype=T, seed=86, scale=0.05)
    outs = []
    for lib_ in (L, S):
        sA = torch.full((rp, H), 0.5, device=dev())
        sBa, sBb = torch.full((H, rp), 0.25, device=dev()), torch.full((H, rp), -0.25, device=dev())
        if lib_ is S:
            x_, dqa_, dqb_, A_, BTa_, BTb_, sA, sBa, sBb = (v.cpu() for v in (x, dqa, dqb, A, BTa, BTb, sA, sBa, sBb))
        else:
            x_, dqa_, dqb_, A_, BTa_, BTb_ = x, dqa, dqb, A, BTa, BTb
            assert L.lora_bwd_fused_ok(x, M, H)
        lib_.lora_bwd_fused(x_, dqa_, dqb_, A_[0:R], A_[16:16 + R], BTa_[0:R], BTb_[16:16 + R], 0.125, 2.0, sA[0:R], sA[16:16 + R], sBa[:, 0:R],
                            sBb[:, 16:16 + R], sBa[:, oc] if bias else None, sBb[:, oc] if bias else None, M, rank_rows=R)
        outs.append((sA.cpu(), sBa.cpu(), sBb.cpu()))
    (gA, gBa, gBb), (wA, wBa, wBb) = outs
    for got, want, what in ((gA, wA, 'dA'), (gBa, wBa, 'dB_q'), (gBb, wBb, 'dB_v')):
        scale = float((want - want.flatten()[0]).abs().max()) + 1e-6
        err = float((got - want).abs().max())
        assert err <= 2e-2 * scale, (what, err, scale)            # t / dt are rounded to bf16 from sums in a different order: a last-place flip moves a product by 2^-8
    # untouched: everything outside the two rank slots and the ones column; rank rows past a LoRA's r see zero weights: zero gradient
    assert torch.equal(gA[32:], torch.full((rp - 32, H), 0.5)) and torch.equal(gBa[:, 16:oc], torch.full((H, oc - 16), 0.25))
    assert torch.equal(gBb[:, :16], torch.full((H, 16), -0.25)) and torch.equal(gBb[:, oc + 1:], torch.full((H, rp - oc - 1), -0.25))
    if R == 8:
        assert torch.equal(gA[8:16], torch.full((8, H), 0.5)) and torch.equal(gBa[:, 8:16], torch.full((H, 8), 0.25))
    if not bias:
        assert torch.equal(gBa[:, oc], torch.full((H,), 0.25))
    assert float((gA[16 + rb:16 + R] - 0.5).abs().max()) < 1e-6 if rb < R else True


def test_ln_dropout_adjoint():
    from adapter4rec_amd import _lib as L
    M, H = 128, 64
    v, gamma, beta = rnd(M, H, seed=46), torch.ones(H, device=dev()), torch.zeros(H, device=dev())
    y, y0, stats = torch.zeros(M, H, device=dev()), torch.zeros(M, H, device=dev()), torch.zeros(M, 2, device=dev())
    L.ln_fwd(v, gamma, beta, 1e-6, y0, stats)
    L.ln_fwd(v, gamma, beta, 1e-6, y, stats, drop_p=0.3, drop_site=9, drop_seed=5)
    kept = y != 0
    assert abs(1 - kept.float().mean().item() - 0.3) < 0.03
    # backward must apply the same mask: feed dy = 1 on kept entries only vs dy = 1 everywhere
    dv_a, dv_b = torch.zeros(M, H, device=dev()), torch.zeros(M, H, device=dev())
    ones = torch.ones(M, H, device=dev())
    L.ln_bwd(ones, v, stats, gamma, dv_a, drop_p=0.3, drop_site=9, drop_seed=5)
    scale = 1.0 / (1.0 - round(0.3 * 65536) / 65536)
    L.ln_bwd(kept.float() * scale, v, stats, gamma, dv_b)
    torch.testing.assert_close(dv_a, dv_b, rtol=1e-4, atol=1e-5)


@pytest.mark.parametrize('dt', ['f32', 'bf16'])
def test_ln_bwd_second_output_through_dropout(dt):
    """a4r_ln_bwd's optional second output = a4r_dropout_apply of its first (same mask index row * H + col; bit for bit in fp32), with and without
    the residual-branch operand; the first output and the column sums are unchanged by it."""
    from adapter4rec_amd import _lib as L
    t = DT[dt]
    M, H = 300, 256
    v, dy, dres = rnd(M, H, dtype=t, seed=61), rnd(M, H, dtype=t, seed=62), rnd(M, H, dtype=t, seed=63)
    gamma, stats = 1 + 0.1 * rnd(H, seed=64), torch.zeros(M, 2, device=dev())
    y = torch.zeros(M, H, dtype=t, device=dev())
    L.ln_fwd(v, gamma, torch.zeros(H, device=dev()), 1e-6, y, stats)
    for res in (None, dres):
        dv_a, dv_b, dh_a, dh_b = (torch.zeros(M, H, dtype=t, device=dev()) for _ in range(4))
        dba, dbb = torch.zeros(H, device=dev()), torch.zeros(H, device=dev())
        L.ln_bwd(dy, v, stats, gamma, dv_a, dres=res, dbias=dba)
        L.dropout_apply(dv_a, dh_a, 0.2, 7, 99)
        L.ln_bwd(dy, v, stats, gamma, dv_b, dres=res, dbias=dbb, dv2=dh_b, drop2_p=0.2, drop2_site=7, drop2_seed=99)
        assert torch.equal(dv_a, dv_b) and torch.equal(dh_a == 0, dh_b == 0)
        if dt == 'f32':
            assert torch.equal(dh_a, dh_b)
        else:                        # the fused launch scales the fp32 value and rounds ONCE; the two-launch form rounds dv first
            torch.testing.assert_close(dh_a.float(), dh_b.float(), rtol=2 ** -7, atol=1e-3)
        torch.testing.assert_close(dba, dbb, rtol=1e-4, atol=1e-4)       # (column sums flushed with fp32 atomics: the order differs from launch to launch -- 1e-5 failed once in ~5 runs)
        assert abs((dh_b == 0).float().mean().item() - 0.2) < 0.02


@pytest.mark.parametrize('dt', ['f32', 'bf16'])
@pytest.mark.parametrize('M,H', [(2048, 768), (40448, 768), (2051, 384), (8 * 256 * 2 + 5, 1024), (16896, 768)])
def test_ln_bwd_param_grads_lean_loads(dt, M, H):
    """a4r_ln_bwd with dgamma / dbeta on >= 2048 rows (trainable LayerNorms of un-adapted sub-layers: full fine-tuning, --finetune_layernorm) runs
    ln_bwd_pg_kernel (8-wave workgroups, one per CU, next row in flight): against the general kernel -- forced by an all-zero additive table -- and torch
    fp32, with / without the residual-branch operand and the second output through a dropout mask (same mask as a4r_dropout_apply); gradients ACCUMULATE."""
    from adapter4rec_amd import _lib as L
    t = DT[dt]
    v, dy, dres = rnd(M, H, dtype=t, seed=91, scale=2.0), rnd(M, H, dtype=t, seed=92), rnd(M, H, dtype=t, seed=93)
    gamma, beta = rnd(H, seed=94) * 0.2 + 1, rnd(H, seed=95) * 0.1
    zero_add = torch.zeros(1, H, device=dev())
    y, st = torch.zeros(M, H, dtype=t, device=dev()), torch.zeros(M, 2, device=dev())
    L.ln_fwd(v, gamma, beta, 1e-6, y, st)
    vr = v.float().clone().requires_grad_(True)
    gr, br = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    torch.nn.functional.layer_norm(vr, (H,), gr, br, 1e-6).backward(dy.float())
    for res, second in ((None, False), (dres, True)):
        outs = []
        for add in (None, zero_add):
            dv, dh = torch.zeros(M, H, dtype=t, device=dev()), torch.zeros(M, H, dtype=t, device=dev())
            dg, db = torch.full((H,), 0.5, device=dev()), torch.full((H,), -0.25, device=dev())
            kw = dict(dv2=dh, drop2_p=0.1, drop2_site=5, drop2_seed=77) if second else {}
            L.ln_bwd(dy, v, st, gamma, dv, dres=res, add=add, dgamma=dg, dbeta=db, **kw)
            outs.append((dv, dh, dg, db))
        (dv_n, dh_n, dg_n, db_n), (dv_g, dh_g, dg_g, db_g) = outs
        tol = dict(rtol=1e-5, atol=1e-5) if dt == 'f32' else dict(rtol=2 ** -7, atol=2 ** -7)
        torch.testing.assert_close(dv_n.float(), dv_g.float(), **tol)
        scale_ = float(dg_g.abs().max()) + 1.0
        torch.testing.assert_close(dg_n, dg_g, rtol=1e-4, atol=2e-5 * scale_ * (M / 2048) ** 0.5)
        torch.testing.assert_close(db_n, db_g, rtol=1e-4, atol=2e-5 * scale_ * (M / 2048) ** 0.5)
        close(dv_n, vr.grad + (res.float() if res is not None else 0), t, f'ln bwd pg M={M} H={H}', atol32=3e-4)
        if dt == 'f32':
            torch.testing.assert_close(dg_n, 0.5 + gr.grad, rtol=2e-4, atol=2e-4 * scale_)
            torch.testing.assert_close(db_n, -0.25 + br.grad, rtol=2e-4, atol=2e-4 * scale_)
        if second:
            assert torch.equal(dh_n == 0, dh_g == 0) and abs((dh_n == 0).float().mean().item() - 0.1) < 0.02
            torch.testing.assert_close(dh_n.float(), dh_g.float(), **tol)
            ref2 = torch.zeros(M, H, dtype=t, device=dev())
            L.dropout_apply(dv_n, ref2, 0.1, 5, 77)
            assert torch.equal(ref2 == 0, dh_n == 0)


def test_rows_idx_copy():
    """a4r_rows_idx_copy: rows by index, any element type (int64 id rows, fp32 embeddings, uint8 images), strided views on both sides, gather and its
    scatter inverse; untouched destination rows keep their contents."""
    from adapter4rec_amd import _lib as L
    g = torch.Generator().manual_seed(9)
    idx = torch.randperm(500, generator=g)[:123].sort().values.to(torch.int32).to(dev())
    for src in (torch.randint(0, 30000, (500, 60), generator=g).to(dev()), rnd(500, 64, seed=3), torch.randint(0, 255, (500, 48), generator=g).to(torch.uint8).to(dev()),
                rnd(500, 72, seed=4)[:, 4:68]):
        comp = torch.zeros(130, src.shape[1] + 16, dtype=src.dtype, device=dev())[:, :src.shape[1]]
        L.rows_idx_copy(src, comp, idx, 123)
        assert torch.equal(comp[:123], src[idx.long()]) and torch.count_nonzero(comp[123:]) == 0
        back = torch.full_like(src, 7)
        L.rows_idx_copy(comp, back, idx, 123, scatter=True)
        want = torch.full_like(src, 7)
        want[idx.long()] = src[idx.long()]
        assert torch.equal(back, want)
    with pytest.raises(RuntimeError):
        L.rows_idx_copy(rnd(8, 6), rnd(8, 6), idx, 4)                       # 24-byte rows


@pytest.mark.parametrize('dt', ['f32', 'bf16'])
def test_gather_scatter_rows(dt):
    from adapter4rec_amd import _lib as L
    t = DT[dt]
    n, S, H = 10, 30, 768
    x = rnd(384, H, dtype=t, seed=51)
    g = torch.zeros(128, H, dtype=t, device=dev())
    L.gather_rows(x, g, n, S)
    assert torch.equal(g[:n], x[0:n * S:S])
    back = torch.zeros_like(x)
    L.scatter_rows(g, back, n, S)
    assert torch.equal(back[0:n * S:S], g[:n])
    assert torch.count_nonzero(back) == torch.count_nonzero(g[:n])


def test_act_bwd_f32():
    from adapter4rec_amd import _lib as L
    dy, pre = rnd(300, 64, seed=52), rnd(300, 64, seed=53)
    for act in (1, 2, 3):
        dx = torch.zeros_like(dy)
        L.act_bwd_f32(dy, pre, dx, act)
        p = pre.clone().requires_grad_(True)
        act_ref(p, act).backward(dy)
        close(dx, p.grad, torch.float32, f'act_bwd {act}')


# ------------------------------------------------------------------ head / optimiser / eval
@pytest.mark.parametrize('cpc', [False, True])
def test_score_bce(cpc):
    from adapter4rec_amd import _lib as L
    B, Ls, E = 6, 21, 64
    emb = rnd(B, Ls, 2, E, seed=61).requires_grad_(True)
    prec = rnd(B, Ls - 1, E, seed=62).requires_grad_(True)
    mask = torch.ones(B, Ls - 1)
    mask[1, :7] = 0
    mask[2, :16] = 0
    mask = mask.to(dev())
    pos, neg = torch.zeros(B, Ls - 1, device=dev()), torch.zeros(B, Ls - 1, device=dev())
    ws = torch.zeros(4, device=dev())
    L.score_bce_fwd(emb.detach(), prec.detach(), mask, pos, neg, ws, B, Ls, E, cpc)
    tp, tn = emb[:, 1:, 0], emb[:, :-1, 1]
    bce = torch.nn.BCEWithLogitsLoss()
    if cpc:
        ps, ns = (prec[:, -1] * tp[:, -1]).sum(-1), (prec[:, -1] * tn[:, -1]).sum(-1)
        loss = bce(ps, torch.ones_like(ps)) + bce(ns, torch.zeros_like(ns))
    else:
        ps, ns = (prec * tp).sum(-1), (prec * tn).sum(-1)
        idx = mask != 0
        loss = bce(ps[idx], torch.ones_like(ps[idx])) + bce(ns[idx], torch.zeros_like(ns[idx]))
        close(pos, ps.detach(), torch.float32, 'pos scores')
        close(neg, ns.detach(), torch.float32, 'neg scores')
    assert abs(ws[0].item() - loss.item()) < 1e-5
    loss.backward()
    d_prec, d_emb = torch.zeros_like(prec), torch.full_like(emb, 7.0)
    L.score_bce_bwd(emb.detach(), prec.detach(), mask, pos, neg, ws, 1.0, d_prec, d_emb, B, Ls, E, cpc)
    close(d_prec, prec.grad, torch.float32, 'd_prec', atol32=1e-6)
    close(d_emb, emb.grad, torch.float32, 'd_emb', atol32=1e-6)
    # input-side pieces
    take = torch.zeros(128, E, device=dev())
    L.take_inputs(emb.detach(), take, B, Ls, E)
    assert torch.equal(take[:B * (Ls - 1)].view(B, Ls - 1, E), emb.detach()[:, :-1, 0])
    d_in = rnd(128, E, seed=63)
    before = d_emb.clone()
    L.emb_grad_add_inputs(d_in, d_emb, B, Ls, E)
    before[:, :-1, 0] += d_in[:B * (Ls - 1)].view(B, Ls - 1, E)
    close(d_emb, before, torch.float32, 'emb_grad_add_inputs')


def test_adam_matches_torch():
    from adapter4rec_amd import _lib as L
    sizes, groups, lrs = [1000, 64, 4096, 17], [2, 2, 3, 1], [5e-5, 1e-4, 1.5e-4, 2e-4]
    n = sum(sizes)
    p = rnd(n, seed=71)
    params = [torch.nn.Parameter(x.clone()) for x in torch.split(p.clone(), sizes)]
    opt = torch.optim.Adam([{'params': [q], 'lr': lrs[g]} for q, g in zip(params, groups)])
    m, v = torch.zeros(n, device=dev()), torch.zeros(n, device=dev())
    seg_end = torch.tensor([sum(sizes[:i + 1]) for i in range(len(sizes))], dtype=torch.int32, device=dev())
    seg_group = torch.tensor(groups, dtype=torch.int32, device=dev())
    glr = torch.tensor(lrs, device=dev())
    for step in range(1, 4):
        g = rnd(n, seed=72 + step)
        for q, gg in zip(params, torch.split(g, sizes)):
            q.grad = gg.clone()
        opt.step()
        L.adam_step(p, g, m, v, seg_end, seg_group, glr, step)
    torch.testing.assert_close(p, torch.cat([q.detach() for q in params]), rtol=1e-5, atol=1e-7)


def test_adam_quads_equal_scalar_kernel():
    """Full fine-tuning steps ~110 M parameters through a4r_adam_step: buffers of >= 2^20 elements on 16-byte addresses take adam4_kernel (four
    parameters per lane) + the scalar kernel on the n % 4 tail.  Same arithmetic per element: bit-identical to the scalar kernel (reached here
    through a view that starts 4 bytes into the buffers), segments of odd lengths straddling the quads."""
    from adapter4rec_amd import _lib as L
    sizes, groups, lrs = [1000003, 5, 64, 2 ** 20 + 1, 18], [0, 2, 1, 3, 1], [5e-5, 1e-4, 1.5e-4, 2e-4]
    n = sum(sizes)
    seg_end = torch.tensor([sum(sizes[:i + 1]) for i in range(len(sizes))], dtype=torch.int32, device=dev())
    seg_group = torch.tensor(groups, dtype=torch.int32, device=dev())
    glr = torch.tensor(lrs, device=dev())
    p0 = rnd(n, seed=74)
    bufs = []
    for off in (0, 1):                                    # off = 1: misaligned views -> the scalar kernel for everything
        p, m, v = [torch.zeros(n + 4, device=dev())[off:off + n] for _ in range(3)]
        p.copy_(p0)
        for step in range(1, 4):
            g = torch.zeros(n + 4, device=dev())[off:off + n]
            g.copy_(rnd(n, seed=75 + step))
            L.adam_step(p, g, m, v, seg_end, seg_group, glr, step)
        bufs.append((p.clone(), m.clone(), v.clone()))
    for a, b in zip(*bufs):
        assert torch.equal(a, b)
    assert not torch.equal(bufs[0][0], p0)


def test_pack_matrices_large_tiled():
    """Matrix lists that hold a large matrix (>= 256 x 256 elements: trainable backbone weights) go through the 64 x 64-tile kernel: plain and
    transposed copies, zero padding, a destination that is a column block of a wider matrix (dst_ld), ragged edge tiles; a small matrix in the list."""
    from adapter4rec_amd import _lib as L
    shapes = [(768, 3072), (3072, 768), (300, 257), (16, 64)]
    flat = rnd(sum(r * c for r, c in shapes), seed=76)
    wide = torch.full((320, 3 * 320), 7.0, dtype=torch.bfloat16, device=dev())
    dsts = [torch.zeros(768, 3072, dtype=torch.bfloat16, device=dev()), torch.zeros(768, 3072, dtype=torch.bfloat16, device=dev()), wide[:, 320:640],
            torch.zeros(64, 64, dtype=torch.bfloat16, device=dev())]
    descs = (L.PackDesc * 4)()
    off = 0
    for i, ((r, c), d, tr, pad) in enumerate(zip(shapes, dsts, (0, 1, 1, 0), ((768, 3072), (768, 3072), (320, 320), (64, 64)))):
        descs[i] = L.PackDesc(off, d.data_ptr(), r, c, pad[0], pad[1], tr, 3 * 320 if i == 2 else 0)
        off += r * c
    raw = torch.frombuffer(bytearray(bytes(descs)), dtype=torch.uint8).to(dev())
    L.pack_matrices(flat, raw, 4, 768 * 3072, L.BF16)
    srcs = torch.split(flat, [r * c for r, c in shapes])
    assert torch.equal(dsts[0], srcs[0].view(768, 3072).bfloat16())
    assert torch.equal(dsts[1], srcs[1].view(3072, 768).t().bfloat16())
    ref = torch.zeros(320, 320, dtype=torch.bfloat16, device=dev())
    ref[:257, :300] = srcs[2].view(300, 257).t().bfloat16()
    assert torch.equal(wide[:, 320:640], ref) and bool((wide[:, :320] == 7).all()) and bool((wide[:, 640:] == 7).all())
    assert torch.equal(dsts[3][:16], srcs[3].view(16, 64).bfloat16()) and torch.count_nonzero(dsts[3][16:]) == 0


def test_pack_matrices():
    import ctypes as C
    from adapter4rec_amd import _lib as L
    flat = rnd(16 * 64 + 768 * 64, seed=73)
    d1 = torch.zeros(64, 64, dtype=torch.bfloat16, device=dev())       # [16,64] -> padded [64,64]
    d2 = torch.zeros(64, 768, dtype=torch.bfloat16, device=dev())      # [768,64] -> transpose [64,768]
    descs = (L.PackDesc * 2)()
    descs[0] = L.PackDesc(0, d1.data_ptr(), 16, 64, 64, 64, 0, 0)
    descs[1] = L.PackDesc(16 * 64, d2.data_ptr(), 768, 64, 64, 768, 1, 0)
    raw = torch.frombuffer(bytearray(bytes(descs)), dtype=torch.uint8).to(dev())
    L.pack_matrices(flat, raw, 2, 64 * 768, L.BF16)
    w1 = flat[:16 * 64].view(16, 64)
    assert torch.equal(d1[:16].float(), w1.bfloat16().float()) and torch.count_nonzero(d1[16:]) == 0
    assert torch.equal(d2.float(), flat[16 * 64:].view(768, 64).t().bfloat16().float())


@pytest.mark.parametrize('E,max_hist', [(64, 22), (128, 22), (256, 22), (512, 22), (64, 264), (128, 102)])
def test_eval_rank(E, max_hist):
    """(E = 256: the parser's default --embedding_dim; 512: instantiated in round 5; histories of up to A4R_EVAL_MAX_HISTORY = 264 ids:
    --max_seq_len up to 255 keeps max_seq_len + 2 of them, preprocess.py:51-59)"""
    from adapter4rec_amd import _lib as L
    assert L.EVAL_MAX_HISTORY == 264
    U, N1 = 37, 1001
    prec, items = rnd(U, E, seed=81), rnd(N1, E, seed=82)
    g = torch.Generator().manual_seed(3)
    target = torch.randint(1, N1, (U,), generator=g).int()
    hist, ptr = [], [0]
    for u in range(U):
        h = torch.randint(1, N1, (max_hist if u == 5 else int(torch.randint(0, max_hist + 1, (1,), generator=g)),), generator=g).tolist()
        h = [x for x in h if x != int(target[u])] if u != 5 else [x if x != int(target[u]) else (x % (N1 - 1)) + 1 for x in h]
        hist += h
        ptr.append(len(hist))
    rank = torch.zeros(U, dtype=torch.int32, device=dev())
    L.eval_rank(prec, items, target.to(dev()), torch.tensor(ptr, dtype=torch.int32, device=dev()),
                torch.tensor(hist + [0], dtype=torch.int32, device=dev()), rank)
    sc = (prec.double() @ items.double().t()).cpu()
    ref = []
    for u in range(U):
        s = sc[u].clone()
        tsc = s[int(target[u])].item()
        s[torch.tensor(hist[ptr[u]:ptr[u + 1]], dtype=torch.long)] = -float('inf')
        ref.append(int((s[1:] > tsc).sum()) + 1)
    got = rank.cpu().tolist()
    assert sum(abs(a - b) for a, b in zip(got, ref)) <= 1, (got, ref)     # fp32 vs fp64 near-ties


# ------------------------------------------------------------------ one-launch adapter + residual(s) + LayerNorm
AD_MODES = {'houlsby': (1, True), 'houlsby_gelu': (2, True), 'compacter': (3, False), 'pfeiffer': (1, False), 'parallel': (1, True)}


def _adapter_case(H, M, seed=90):
    t, dp = torch.bfloat16, 64
    a, o = rnd(M, H, dtype=t, seed=seed + 1), rnd(M, H, dtype=t, seed=seed + 2)
    Wd, Wu = rnd(dp, H, dtype=t, scale=0.05, seed=seed + 3), rnd(H, dp, dtype=t, scale=0.05, seed=seed + 4)
    bd, bu = rnd(dp, seed=seed + 5) * 0.1, rnd(H, seed=seed + 6) * 0.1
    gamma, beta = rnd(H, seed=seed + 7) * 0.1 + 1, rnd(H, seed=seed + 8) * 0.1
    return a, o, Wd, Wu, bd, bu, gamma, beta


@pytest.mark.parametrize('H', [128, 256, 512, 768, 1024])
@pytest.mark.parametrize('mode', list(AD_MODES))
def test_adapter_ln_fwd(H, mode):
    """a4r_adapter_ln_fwd vs torch fp32 and vs the three-launch form (a4r_gemm_nt x 2 + a4r_ln_fwd) it replaces; M = 16 x 301
    rows: more tiles than workgroups, a ragged last round, every wave-to-column mapping (H / 8 columns per wave)."""
    from adapter4rec_amd import _lib as L
    act, inner = AD_MODES[mode]
    M, dp, t = 16 * 301, 64, torch.bfloat16
    a, o, Wd, Wu, bd, bu, gamma, beta = _adapter_case(H, M)
    mk = lambda c: torch.zeros(M, c, dtype=t, device=dev())
    zp, z, v, y, stats = mk(dp), mk(dp), mk(H), mk(H), torch.zeros(M, 2, device=dev())
    if mode == 'parallel':
        R1, R2 = o, a                                          # up + (dense + input) + input: the adapter reads the sub-layer input
    else:
        R1, R2 = (a, o) if inner else (o, None)
    L.adapter_ln_fwd(a, R1, R2, Wd, bd, Wu, bu, gamma, beta, 1e-12, act, zp, z, v, y, stats)
    zp_r = a.float() @ Wd.float().t() + bd
    z_r = act_ref(zp_r, act)
    v_r = z_r.to(t).float() @ Wu.float().t() + bu + R1.float() + (R2.float() if R2 is not None else 0)
    vq = v_r                                                  # LayerNorm runs on the fp32 sum (round 4; rounds 1 - 3: on the bf16-rounded v)
    y_r = torch.nn.functional.layer_norm(vq, (H,), gamma, beta, 1e-12)
    close(zp, zp_r, t, 'zp')
    close(z, z_r, t, 'z')
    close(v, v_r, t, 'v')
    close(y, y_r, t, 'y')
    close(stats[:, 0], vq.mean(-1), torch.float32, 'mean', atol32=2e-3, rtol32=1e-3)
    close(stats[:, 1], torch.rsqrt(vq.var(-1, unbiased=False) + 1e-12), torch.float32, 'rstd', atol32=2e-3, rtol32=2e-3)
    # the launches it replaces, same inputs: outputs agree to bf16 rounding of the stored intermediates
    Mp = 16 * 304                                             # (a4r_gemm_nt wants M % 128 == 0: padded copies)
    pad = lambda x: torch.cat([x, torch.zeros(Mp - M, x.shape[1], dtype=x.dtype, device=dev())])
    a2, r1, r2 = pad(a), pad(R1), (pad(R2) if R2 is not None else None)
    if R1 is a:
        r1 = a2
    if R2 is a:
        r2 = a2
    mk2 = lambda c: torch.zeros(Mp, c, dtype=t, device=dev())
    zp2, z2, v2, y2, st2 = mk2(dp), mk2(dp), mk2(H), mk2(H), torch.zeros(Mp, 2, device=dev())
    L.gemm_nt(a2, Wd, z2, bias=bd, C2=zp2, act=act)
    L.gemm_nt(z2, Wu, v2, bias=bu, R1=r1, R2=r2)
    L.ln_fwd(v2, gamma, beta, 1e-12, y2, st2)
    close(zp, zp2[:M], t, 'zp vs 3 launches', rtol16=1e-2, atol16=1e-2)
    close(v, v2[:M], t, 'v vs 3 launches', rtol16=1e-2, atol16=2e-2)
    close(y, y2[:M], t, 'y vs 3 launches', rtol16=1e-2, atol16=3e-2)
    # e4m3 form of y (+ per-row scale) from the same launch, with and without the bf16 copy: the a4r_ln_fwd_fp8 arithmetic
    for keep_y in (True, False):
        y8, ys = torch.zeros(M, H, dtype=torch.uint8, device=dev()), torch.zeros(M, device=dev())
        yb = mk(H) if keep_y else None
        L.adapter_ln_fwd(a, R1, R2, Wd, bd, Wu, bu, gamma, beta, 1e-12, act, mk(dp), mk(dp), mk(H), yb, torch.zeros(M, 2, device=dev()), y8=y8, ys=ys)
        if keep_y:
            assert torch.equal(yb, y)
        amax = y_r.abs().amax(1)
        close(ys, amax / 448.0, torch.float32, 'fp8 row scale', atol32=1e-4, rtol32=2e-2)
        deq = y8.view(torch.float8_e4m3fn).float() * ys[:, None]
        assert float((deq - y_r).abs().max() / amax.max()) < 0.07                      # e4m3: 3 mantissa bits
        assert int(y8.view(torch.float8_e4m3fn).float().abs().max()) == 448            # every row uses the full range


@pytest.mark.parametrize('H', [128, 256, 512, 768])
@pytest.mark.parametrize('act,inner,sums,drop', [(1, True, 'b', 0.1), (2, True, 'gb', 0.0), (3, False, 'b', 0.25), (1, False, 'gb', 0.0), (1, True, '', 0.1)])
def test_adapter_ln_bwd(H, act, inner, sums, drop):
    """a4r_adapter_ln_bwd vs the three launches it replaces (a4r_ln_bwd | a4r_gemm_nt dact | a4r_gemm_nt + residual + dropout: SAME
    dropout mask, regenerated from (seed, site, row * H + col)) and vs torch fp32; column sums dgamma / dbeta / dbias."""
    from adapter4rec_amd import _lib as L
    M, Mp, dp, t = 16 * 301, 16 * 304, 64, torch.bfloat16
    _, _, Wd, Wu, bd, bu, gamma, beta = _adapter_case(H, Mp, seed=120)
    dy, v = rnd(Mp, H, dtype=t, seed=131), rnd(Mp, H, dtype=t, scale=1.5, seed=132)
    zp = rnd(Mp, dp, dtype=t, seed=133)
    WuT, WdT = Wu.t().contiguous(), Wd.t().contiguous()
    vf = v.float()
    mean = vf.mean(-1)
    rstd = torch.rsqrt(vf.var(-1, unbiased=False) + 1e-12)
    stats = torch.stack([mean, rstd], 1).contiguous()
    mk = lambda c: torch.zeros(Mp, c, dtype=t, device=dev())
    vec = lambda: torch.zeros(H, device=dev())
    dv, dzp, dh = mk(H), mk(dp), mk(H)
    dg, db, dbi = (vec() if 'g' in sums else None), (vec() if 'g' in sums else None), (vec() if 'b' in sums else None)
    dbd = torch.zeros(dp, device=dev()) if 'b' in sums else None
    L.adapter_ln_bwd(dy, v, stats, gamma, None, zp, act, WuT, WdT, inner, dv, dzp, dh, dgamma=dg, dbeta=db, dbias=dbi, M=M,
                     drop_p=drop, drop_site=9, drop_seed=4242, dbd=dbd)
    assert float(dv[M:].abs().max()) == 0 and float(dh[M:].abs().max()) == 0        # rows >= M untouched
    if dbd is not None:                      # the down-projection's bias gradient = column sums of dzp
        ref_bd = dzp[:M].float().sum(0)
        close(dbd, ref_bd, torch.float32, 'dbd vs colsum(dzp)', atol32=2e-2 * max(1.0, float(ref_bd.abs().max())), rtol32=1e-2)
    # the three launches
    dv2, dzp2, dh2 = mk(H), mk(dp), mk(H)
    dg2, db2, dbi2 = (vec() if 'g' in sums else None), (vec() if 'g' in sums else None), (vec() if 'b' in sums else None)
    L.ln_bwd(dy, v, stats, gamma, dv2, dgamma=dg2, dbeta=db2, dbias=dbi2, M=M)
    L.gemm_nt(dv2, WuT, dzp2, Pre=zp, dact=act)
    L.gemm_nt(dzp2, WdT, dh2, R1=dv2 if inner else None, drop_p=drop, drop_site=9, drop_seed=4242)
    close(dv[:M], dv2[:M], t, 'dv vs ln_bwd', rtol16=1e-2, atol16=1e-2)
    close(dzp[:M], dzp2[:M], t, 'dzp vs 3 launches', rtol16=2e-2, atol16=2e-2)
    if drop:
        assert torch.equal(dh[:M] == 0, dh2[:M] == 0), 'dropout mask differs from the GEMM epilogue\'s'
        assert 0.5 * drop < float((dh[:M] == 0).float().mean()) < 1.5 * drop
    close(dh[:M], dh2[:M], t, 'dh vs 3 launches', rtol16=2e-2, atol16=3e-2)
    for got, ref, nm in ((dg, dg2, 'dgamma'), (db, db2, 'dbeta'), (dbi, dbi2, 'dbias')):
        if got is not None:
            close(got, ref, torch.float32, nm, atol32=2e-2 * max(1.0, float(ref.abs().max())), rtol32=1e-2)
    # torch fp32 on the same (bf16) inputs
    xh = (vf[:M] - mean[:M, None]) * rstd[:M, None]
    gq = dy[:M].float() * gamma
    dv_r = rstd[:M, None] * (gq - gq.mean(-1, keepdim=True) - xh * (gq * xh).mean(-1, keepdim=True))
    close(dv[:M], dv_r, t, 'dv vs torch')
    pre = zp[:M].float().requires_grad_(True)
    act_ref(pre, act).sum().backward()
    dzp_r = (dv[:M].float() @ Wu.float()) * pre.grad
    close(dzp[:M], dzp_r, t, 'dzp vs torch')
    dh_r = dzp[:M].float() @ Wd.float() + (dv[:M].float() if inner else 0)
    keep = dh[:M] != 0
    scale = 1.0 / (1.0 - round(drop * 65536) / 65536) if drop else 1.0
    close(dh[:M][keep], (dh_r * scale)[keep], t, 'dh vs torch')
    if dbi is not None:
        close(dbi, dv_r.sum(0), torch.float32, 'dbias vs torch', atol32=3e-2 * max(1.0, float(dv_r.sum(0).abs().max())), rtol32=2e-2)
    if dg is not None:
        close(dg, (dy[:M].float() * xh).sum(0), torch.float32, 'dgamma vs torch', atol32=1e-2 * float((dy[:M].float() * xh).sum(0).abs().max()), rtol32=1e-2)


def test_adapter_ln_rejects():
    from adapter4rec_amd import _lib as L
    t = torch.bfloat16
    a, o, Wd, Wu, bd, bu, gamma, beta = _adapter_case(192, 64)             # width without an instantiation
    mk = lambda c: torch.zeros(64, c, dtype=t, device=dev())
    with pytest.raises(RuntimeError):
        L.adapter_ln_fwd(a, a, o, Wd, bd, Wu, bu, gamma, beta, 1e-12, 1, mk(64), mk(64), mk(192), mk(192), torch.zeros(64, 2, device=dev()))
    a, o, Wd, Wu, bd, bu, gamma, beta = _adapter_case(128, 64)
    third = mk(128)
    with pytest.raises(RuntimeError):                                      # three distinct streamed tensors
        L.adapter_ln_fwd(a, o, third, Wd, bd, Wu, bu, gamma, beta, 1e-12, 1, mk(64), mk(64), mk(128), mk(128), torch.zeros(64, 2, device=dev()))
    # every other argument check of the two entry points (host side: nothing is launched): each call differs from a valid one in ONE respect, must
    # raise, and leaves the sentinel-filled outputs as they were
    S, M = -768.0, 64

    def args(H=128, d=64, dt=t):
        a, o, Wd, Wu, bd, bu, gamma, beta = _adapter_case(H, M)
        k = dict(a=a.to(dt), o=o.to(dt), Wd=Wd[:d].contiguous().to(dt), Wu=Wu[:, :d].contiguous().to(dt), bd=bd[:d].contiguous(), bu=bu, gamma=gamma, beta=beta)
        full = lambda r, c, dtype=dt, s=S: torch.full((r, c), s, dtype=dtype, device=dev())
        k.update(zp=full(M, 64), z=full(M, 64), v=full(M, H), y=full(M, H), st=full(M, 2, torch.float32), dv=full(M, H), dzp=full(M, 64), dh=full(M, H),
                 dg=full(1, H, torch.float32)[0], dbi=full(1, H, torch.float32)[0], y8=full(M, H, torch.uint8, 0xA5), ys=full(1, M, torch.float32)[0],
                 p4=full(M, H // 2, torch.int8, -77), dy=a.to(dt), vin=o.to(dt), zpin=rnd(M, 64, dtype=dt, seed=5), dres=rnd(M, H, dtype=dt, seed=6),
                 stin=torch.ones(M, 2, device=dev()))
        return k
    outs = ('zp', 'z', 'v', 'y', 'st', 'dv', 'dzp', 'dh', 'dg', 'dbi', 'ys')

    def fwd(k, **kw):
        p = dict(dict(A=k['a'], R1=k['a'], R2=k['o'], zp=k['zp'], z=k['z'], v=k['v'], y=k['y'], M=None, extra={}), **kw)
        L.adapter_ln_fwd(p['A'], p['R1'], p['R2'], k['Wd'], k['bd'], k['Wu'], k['bu'], k['gamma'], k['beta'], 1e-12, 1, p['zp'], p['z'], p['v'], p['y'], k['st'],
                         M=p['M'], **p['extra'])

    def bwd(k, **kw):
        p = dict(dict(dy=k['dy'], v=k['vin'], dres=None, dv=k['dv'], dh=k['dh'], M=None, extra={}), **kw)
        L.adapter_ln_bwd(p['dy'], p['v'], k['stin'], k['gamma'], p['dres'], k['zpin'], 1, k['Wu'].t().contiguous(), k['Wd'].t().contiguous(), True,
                         p['dv'], k['dzp'], p['dh'], M=p['M'], **p['extra'])

    def rejected(k, call, what, **kw):
        with pytest.raises(RuntimeError):
            call(k, **kw)
        torch.cuda.synchronize()
        for nm in outs:
            assert bool((k[nm] == S).all()), f'{what}: {nm} was written'
        assert bool((k['y8'] == 0xA5).all()) and bool((k['p4'] == -77).all()), f'{what}: a byte output was written'

    k = args()
    fwd(k)                                                                 # the base call IS valid (and so is its backward)
    bwd(k)
    assert not bool((k['y'] == S).any()) and not bool((k['dh'] == S).any())
    wide = lambda x, extra, off=0: torch.cat([x, torch.zeros(x.shape[0], extra, dtype=x.dtype, device=dev())], 1)[:, off:off + x.shape[1]]
    for call in (fwd, bwd):
        nm = call.__name__
        rejected(args(), call, f'{nm} M % 16', M=40)
        rejected(args(), call, f'{nm} M = 0', M=0)
        rejected(args(d=32), call, f'{nm} d != 64')
        rejected(args(dt=torch.float32), call, f'{nm} fp32 operands')
    k = args()
    rejected(k, fwd, 'fwd lda % 8', A=wide(k['a'], 4), R1=k['o'], R2=None)
    k = args()
    rejected(k, fwd, 'fwd ldy % 8', y=torch.full((M, 132), S, dtype=t, device=dev())[:, :128])
    k = args()
    rejected(k, fwd, 'fwd A off by 4 elements', A=wide(k['a'], 8, 4), R1=k['o'], R2=None)
    k = args()
    rejected(k, fwd, 'fwd v off by 4 elements', v=torch.full((M, 136), S, dtype=t, device=dev())[:, 4:132])
    k = args()
    rejected(k, bwd, 'bwd lddy % 8', dy=wide(k['dy'], 4))
    k = args()
    rejected(k, bwd, 'bwd dres off by 4 elements', dres=wide(k['dres'], 8, 4))
    k = args()
    rejected(k, bwd, 'bwd dh off by 4 elements', dh=torch.full((M, 136), S, dtype=t, device=dev())[:, 4:132])
    rejected(args(H=1024), bwd, 'bwd H = 1024')
    k = args()
    rejected(k, bwd, 'beta_y with dres', dres=k['dres'], extra=dict(beta_y=k['beta']))
    k = args()
    rejected(k, bwd, 'beta_y with dgamma', extra=dict(beta_y=k['beta'], dgamma=k['dg']))
    k = args()
    bwd(k, extra=dict(beta_y=k['beta'], dbias=k['dbi']))                    # (beta_y alone, with dbias, is an instantiation)
    k = args()
    rejected(k, fwd, 'y8 without ys', extra=dict(y8=k['y8']))
    k = args()
    rejected(k, fwd, 'nibble plane with ld < H / 2', extra=dict(y32=k['p4'].as_strided((M, 64), (60, 1))))


# ------------------------------------------------------------------ fp8 (OCP e4m3fn) operands
def _q8_ref(x):
    """host fp32 (IEEE divide: torch's device kernels turn tensor / scalar into a multiplication by the reciprocal)"""
    d = x.device
    x = x.detach().float().cpu()
    amax = x.abs().amax(1)
    inv = torch.where(amax > 0, torch.tensor(448.0) / amax, torch.zeros_like(amax))
    return (x * inv[:, None]).to(torch.float8_e4m3fn).to(d), torch.where(amax > 0, amax / torch.tensor(448.0), torch.ones_like(amax)).to(d)


@pytest.mark.parametrize('dt', ['bf16', 'f32'])
@pytest.mark.parametrize('H', [128, 768, 1024, 3072])
def test_quant_rows_fp8(dt, H):
    """a4r_quant_rows_fp8 vs torch's float8_e4m3fn cast of the same scaled row: bit-exact (same RNE rounding, correctly rounded fp32
    scaling), incl. an all-zero row."""
    from adapter4rec_amd import _lib as L
    M, t = 517, DT[dt]
    x = rnd(M, H, dtype=t, scale=2.0, seed=H + 1)
    x[3] = 0
    x[5, 7] = 300.0
    q = torch.zeros(M, H, dtype=torch.uint8, device=dev())
    sc = torch.zeros(M, device=dev())
    L.quant_rows_fp8(x, q, sc)
    qr, sr = _q8_ref(x.float())
    assert torch.equal(sc, sr)
    assert torch.equal(q, qr.view(torch.uint8)), int((q != qr.view(torch.uint8)).sum())
    deq = q.view(torch.float8_e4m3fn).float() * sc[:, None]
    assert float(((deq - x.float()).abs() / x.float().abs().clamp_min(1e-3 * float(x.float().abs().max()))).max()) < 2 ** -3
    assert torch.equal(q[3], torch.zeros_like(q[3])) and float(sc[3]) == 1.0


def test_ln_fwd_fp8_output():
    from adapter4rec_amd import _lib as L
    M, H, t = 640, 768, torch.bfloat16
    v = rnd(M, H, dtype=t, scale=1.5, seed=7)
    gamma, beta = rnd(H, seed=8) * 0.1 + 1, rnd(H, seed=9) * 0.1
    y, y2 = torch.zeros(M, H, dtype=t, device=dev()), torch.zeros(M, H, dtype=t, device=dev())
    st, st2 = torch.zeros(M, 2, device=dev()), torch.zeros(M, 2, device=dev())
    y8 = torch.zeros(M, H, dtype=torch.uint8, device=dev())
    ys = torch.zeros(M, device=dev())
    L.ln_fwd(v, gamma, beta, 1e-12, y, st)
    L.ln_fwd(v, gamma, beta, 1e-12, y2, st2, y8=y8, ys=ys)
    assert torch.equal(y, y2) and torch.equal(st, st2)              # the bf16 output is unchanged by the extra output
    ref = torch.nn.functional.layer_norm(v.float(), (H,), gamma, beta, 1e-12)
    deq = y8.view(torch.float8_e4m3fn).float() * ys[:, None]
    close(ys, ref.abs().amax(1) / 448, torch.float32, 'row scale', atol32=1e-5, rtol32=1e-4)
    assert float((deq - ref).abs().max()) <= 2 ** -4 * float(ref.abs().max()) + 1e-6
    L.ln_fwd(v, gamma, beta, 1e-12, None, None, y8=y8, ys=ys)       # y and stats optional


@pytest.mark.parametrize('M,N,K,act', [(256, 256, 128, 0), (512, 768, 768, 0), (256 * 9, 2304, 768, 0), (256 * 5, 3072, 768, 2), (256 * 3, 768, 3072, 0)])
def test_gemm_fp8(M, N, K, act):
    """a4r_gemm_nt with e4m3 operands + per-row scales vs the fp32 product of the DEQUANTISED operands (what the kernel computes up to
    accumulation order), bias / GELU + derivative epilogue included; and within fp8 rounding of the unquantised product."""
    from adapter4rec_amd import _lib as L
    t = torch.bfloat16
    A, B = rnd(M, K, scale=1.0, seed=M + 3), rnd(N, K, scale=0.05, seed=N + 5)
    A[:, 0] *= 8                                                # rows with very different scales
    Aq, As = _q8_ref(A)
    Bq, Bs = L.quantize_weight_fp8(B)
    bias = rnd(N, seed=11) * 0.1
    C = torch.zeros(M, N, dtype=t, device=dev())
    C2 = torch.zeros_like(C) if act else None
    L.gemm_nt(Aq.view(torch.uint8), Bq, C, bias=bias, C2=C2, act=act, c2_deriv=bool(act), scale_a=As, scale_b=Bs)
    ref = (Aq.float() * As[:, None]) @ (Bq.view(torch.float8_e4m3fn).float() * Bs[:, None]).t() + bias
    if act:
        pre = ref.clone().requires_grad_(True)
        act_ref(pre, act).sum().backward()
        close(C2, pre.grad, t, 'fp8 gemm gelu derivative')
        ref = act_ref(ref, act)
    close(C, ref, t, 'fp8 gemm vs dequantised product')
    full = A @ B.t() + bias
    if act:
        full = act_ref(full, act)
    err = float((C.float() - full).abs().max() / full.abs().max())
    assert err < 6e-2, err                                       # e4m3: 2^-4 per element, averaged down by the contraction


def test_gemm_fp8_rejects():
    from adapter4rec_amd import _lib as L
    A = torch.zeros(256, 128, dtype=torch.uint8, device=dev())
    B = torch.zeros(256, 128, dtype=torch.uint8, device=dev())
    C = torch.zeros(256, 256, dtype=torch.bfloat16, device=dev())
    one = torch.ones(256, device=dev())
    with pytest.raises(RuntimeError):
        L.gemm_nt(A, B, C)                                       # no scales
    with pytest.raises(RuntimeError):
        L.gemm_nt(A[:128], B, C[:128], scale_a=one, scale_b=one)     # M % 256


# ------------------------------------------------------------------ parameter-side kernels (a4r_params.hip)
@pytest.mark.parametrize('dt', ['bf16', 'f32'])
@pytest.mark.parametrize('r', [0, 4, 8])
def test_lora_merge(dt, r):
    from adapter4rec_amd import _lib as L
    t, H = DT[dt], 192
    W, A, B = rnd(H, H, seed=1), rnd(max(r, 1), H, seed=2), rnd(H, max(r, 1), seed=3)
    big, bigT = torch.zeros(3 * H, H, dtype=t, device=dev()), torch.zeros(H, 3 * H, dtype=t, device=dev())
    L.lora_merge(W, A[:r] if r else None, B[:, :r].contiguous() if r else None, 1.0 / max(r, 1), big[H:2 * H], bigT[:, H:2 * H], r)
    ref = W + (B[:, :r] @ A[:r]) / max(r, 1) if r else W
    close(big[H:2 * H], ref, t, 'merged rows')
    close(bigT[:, H:2 * H], ref.t(), t, 'merged transpose')
    assert float(big[:H].abs().max()) == 0 and float(bigT[:, 2 * H:].abs().max()) == 0      # the neighbouring slots are untouched


@pytest.mark.parametrize('dt', ['bf16', 'f32'])
def test_lora_merge_batch_tiled_and_elementwise(dt):
    """a4r_lora_merge_batch over a mixed table: 768 x 768 projections (r = 8, 12) and a 64 x 64 one take the 64 x 64-tile path (whole-row pieces, the
    transposed copy through LDS), a 192 x 96 one the element-wise path; rows and transposed columns land in slots of packed operands, neighbours untouched."""
    from adapter4rec_amd import _lib as L
    t = DT[dt]
    shapes = [(768, 768, 8), (768, 768, 12), (64, 64, 4), (192, 96, 8)]
    ents, want = [], []
    for n, (o, i, r) in enumerate(shapes):
        W, A, B = rnd(o, i, seed=10 + n), rnd(r, i, seed=20 + n), rnd(o, r, seed=30 + n)
        big, bigT = torch.zeros(3 * o, i + 8, dtype=t, device=dev()), torch.zeros(i, 3 * o + 8, dtype=t, device=dev())
        ents.append((W, A, B, 2.0 / r, big[o:2 * o, :i], bigT[:, o:2 * o], r))
        want.append((W + (B @ A) * (2.0 / r), big, bigT, o, i))
    L.lora_merge_batch(L.lora_table(ents, dev()))
    for ref, big, bigT, o, i in want:
        close(big[o:2 * o, :i], ref, t, 'merged rows')
        close(bigT[:, o:2 * o], ref.t(), t, 'merged transpose')
        assert float(big[:o].abs().max()) == 0 and float(big[2 * o:].abs().max()) == 0 and float(big[:, i:].abs().max()) == 0
        assert float(bigT[:, :o].abs().max()) == 0 and float(bigT[:, 2 * o:].abs().max()) == 0


def test_phm_build_and_backward_vs_autograd():
    """a4r_phm_build / a4r_phm_bwd vs the reference's construction (model/layers.py:10-22,150-160, kronecker.py:23-34) through
    torch autograd: two PHMLinear (768 -> 64, 64 -> 768) sharing one rule, gradient matrices read from zero-padded scratch."""
    from adapter4rec_amd import _lib as L
    from adapter4rec_amd.model.modules import PHMLinear
    n = 4
    torch.manual_seed(5)
    rule = torch.nn.Parameter(torch.randn(n, n, n) * 0.3)
    mods = [PHMLinear(768, 48, n), PHMLinear(48, 768, n)]
    for m in mods:
        m.set_phm_rule(rule)
    leaves = [rule] + [q for m in mods for q in (m.W_left, m.W_right)]
    sizes = [q.numel() for q in leaves]
    offs = [sum(sizes[:i]) for i in range(len(sizes))]
    flat = torch.cat([q.detach().reshape(-1) for q in leaves]).to(dev())
    eff = torch.zeros(2 * 768 * 48, device=dev())
    G = [torch.randn(64, 768, device=dev()), torch.randn(768, 64, device=dev())]          # zero-padded scratch shapes (48 -> 64)
    G[0][48:] = 0
    G[1][:, 48:] = 0
    ents = [L.PhmDesc(offs[0], offs[1], offs[2], 0, G[0].data_ptr(), G[0].stride(0), 768, 48, n, 0),
            L.PhmDesc(offs[0], offs[3], offs[4], 768 * 48, G[1].data_ptr(), G[1].stride(0), 48, 768, n, 0)]
    tab = L.desc_table(ents, dev())
    L.phm_build(flat, tab, 2, eff)
    def effective_weight(m):
        # nn.Linear-style [out, in] matrix of y = x @ sum_i kron(rule[i], W_left[i] @ W_right[i]) (PHMLinear.forward, Downstream/Text/model/modules.py:258-300)
        w = torch.bmm(m.W_left, m.W_right)
        kron = (m.phm_rule[:, :, None, :, None] * w[:, None, :, None, :]).reshape(m.phm_dim, m.in_features, m.out_features)
        return kron.sum(0).t()
    E = [effective_weight(m) for m in mods]                      # [out, in]
    close(eff[:768 * 48].view(48, 768), E[0].detach(), torch.float32, 'E down', atol32=1e-5)
    close(eff[768 * 48:].view(768, 48), E[1].detach(), torch.float32, 'E up', atol32=1e-5)
    grads = torch.zeros_like(flat)
    L.phm_bwd(flat, tab, 2, grads)
    ref = torch.autograd.grad(E, leaves, [G[0][:48].cpu(), G[1][:, :48].cpu().contiguous()])
    for q, o, r in zip(leaves, offs, ref):
        close(grads[o:o + q.numel()], r.reshape(-1), torch.float32, 'phm grad', atol32=2e-3 * max(1.0, float(r.abs().max())), rtol32=2e-3)


def test_unpack_add_and_scatter_fill():
    from adapter4rec_amd import _lib as L
    a, b = rnd(64, 96, seed=1), rnd(1, 64, seed=2)
    target = rnd(5000, seed=3)
    before = target.clone()
    ents = [L.AddDesc(a.data_ptr(), 100, 16, 80, a.stride(0), 0.5), L.AddDesc(b.data_ptr(), 3000, 1, 16, b.stride(0), 1.0)]
    L.unpack_add(target, L.desc_table(ents, dev()), 2, 16 * 80)
    exp = before.clone()
    exp[100:100 + 16 * 80] += 0.5 * a[:16, :80].reshape(-1)
    exp[3000:3016] += b[0, :16]
    close(target, exp, torch.float32, 'unpack_add', atol32=1e-6)
    for t in (torch.bfloat16, torch.float32):
        src = rnd(40, 128, dtype=t, seed=4)
        dst = rnd(40 * 7 + 56, 128, dtype=t, seed=5)
        tail = dst[280:].clone()
        L.scatter_rows_fill(src, dst, 40, 7, 280)
        ref = torch.zeros(280, 128, dtype=t, device=dev())
        ref[0:280:7] = src
        assert torch.equal(dst[:280], ref) and torch.equal(dst[280:], tail)
    z = rnd(1000, seed=6)
    L.zero(z[100:200])
    assert float(z[100:200].abs().max()) == 0 and float(z[:100].abs().min()) > 0


def test_gemm_tail_panels_split_launch():
    """777 tiles on 256 CUs.  Despite its name this is no split launch any more: gemm_tail_plan(66304, 768) == (256, 1), so the last 3 row
    panels run as 32-row short tiles INSIDE the one 256-tile launch (a4r_gemm_rows_256 returns M; test_gemm_tail_plan_properties).  Results
    and the dropout mask must equal the 128-tile kernel's (variant 1).  The split launch itself (split_rows, drop_row0), reachable only
    under gemm_tail_max(0), is tested in tests/test_gemm_routes_gpu.py (route 'split')."""
    from adapter4rec_amd import _lib as L
    M, N, K = 259 * 256, 768, 2304
    A = rnd(M, K, dtype=torch.bfloat16, seed=71)
    B = rnd(N, K, dtype=torch.bfloat16, scale=0.05, seed=72)
    R1 = rnd(M, N, dtype=torch.bfloat16, seed=73)
    bias = rnd(N, seed=74)
    outs = []
    for v in (2, 1):
        L.gemm_variant(v)
        C = torch.zeros(M, N, dtype=torch.bfloat16, device=dev())
        C2 = torch.zeros_like(C)
        L.gemm_nt(A, B, C, bias=bias, R1=R1, C2=C2, act=2, drop_p=0.25, drop_site=5, drop_seed=99, drop_first=True)
        outs.append((C, C2))
    L.gemm_variant(2)
    (c_a, c2_a), (c_b, c2_b) = outs
    assert torch.equal((c_a == R1), (c_b == R1))                      # identical dropout pattern, tail rows included
    close(c_a, c_b, torch.bfloat16, 'split vs single launch', rtol16=2e-2, atol16=2e-2)
    close(c2_a[-768:], c2_b[-768:], torch.bfloat16, 'tail C2', rtol16=2e-2, atol16=2e-2)
    assert float((c_a[-768:] != R1[-768:]).float().mean()) > 0.5     # the tail was really written


@pytest.mark.parametrize('dt', ['f32', 'bf16'])
@pytest.mark.parametrize('dh,nh', [(64, 2), (32, 4)])
def test_attn_packed_items_equal_rectangular(dt, dh, nh):
    """a4r_attn_t.offsets (ABI 407): items of DIFFERENT token counts stored back to back.  Forward and backward (the generic and the transposed-read
    bf16 kernel) must equal the rectangular form [n_items, S] with the pad keys masked, on the attended rows, bit for bit in the forward and to
    fp32 summation order in the backward (same kernels, same per-item arithmetic); dropout draws the same (item, head, query, key) counters."""
    from adapter4rec_amd import _lib as L
    t = DT[dt]
    n, S, H = 37, 30, nh * dh
    g = torch.Generator().manual_seed(7)
    lens = torch.randint(1, S + 1, (n,), generator=g)
    lens[0], lens[1] = S, 1
    off = torch.zeros(n + 1, dtype=torch.int32)
    off[1:] = torch.cumsum(lens, 0).int()
    Mtok = int(off[-1])
    valid = (torch.arange(S)[None, :] < lens[:, None])
    rect = rnd(n * S, 3 * H, dtype=t, seed=11)
    dout_r = rnd(n * S, H, dtype=t, seed=12)
    rows = valid.reshape(-1).nonzero().flatten().to(dev())
    packed, dout_p = rect[rows].contiguous(), dout_r[rows].contiguous()
    km = valid.float().to(dev())
    offd = off.to(dev())
    for p_drop in (0.0, 0.1):
        kw = dict(drop_p=p_drop, drop_site=16, drop_seed=99)
        o_r = torch.zeros(n * S, H, dtype=t, device=dev())
        o_p = torch.zeros(Mtok, H, dtype=t, device=dev())
        L.attn_fwd(rect, o_r, km, n, S, nh, dh, 0, H, 2 * H, False, dh ** -0.5, -1e9, **kw)
        L.attn_fwd(packed, o_p, None, n, S, nh, dh, 0, H, 2 * H, False, dh ** -0.5, -1e9, offsets=offd, **kw)
        assert torch.equal(o_p, o_r[rows]), (dt, dh, p_drop)
        d_r = torch.zeros(n * S, 3 * H, dtype=t, device=dev())
        d_p = torch.zeros(Mtok, 3 * H, dtype=t, device=dev())
        do_r = dout_r * km.reshape(-1, 1).to(t)                   # pad queries carry no gradient in the packed form: they do not exist
        L.attn_bwd(rect, do_r, d_r, km, n, S, nh, dh, 0, H, 2 * H, False, dh ** -0.5, -1e9, **kw)
        L.attn_bwd(packed, dout_p, d_p, None, n, S, nh, dh, 0, H, 2 * H, False, dh ** -0.5, -1e9, offsets=offd, **kw)
        close(d_p, d_r[rows], t, f'packed attention backward {dt} dh={dh} p={p_drop}')


@pytest.mark.parametrize('K', [192, 256, 768])
def test_gemm256_many_tiles_per_workgroup(K):
    """540 output tiles on 256 persistent workgroups: every workgroup walks 2 - 3 tiles, so the unit stream continues ACROSS tiles
    (K / 64 even) or a prologue is issued per tile (K / 64 odd: K = 192), workgroups with a tile of slack start late, and each epilogue
    instantiation of the training step (plain, dropout, residual, GELU + 8-bit derivative, * 8-bit derivative) runs on tiles that are
    not a workgroup's first.  Checked against the 128-tile kernel (same epilogue code, one tile per workgroup) and fp32 torch."""
    from adapter4rec_amd import _lib as L
    t = torch.bfloat16
    M, N = 180 * 256, 768
    A, B = rnd(M, K, dtype=t, seed=81), rnd(N, K, dtype=t, scale=0.05, seed=82)
    bias, R1 = rnd(N, seed=83), rnd(M, N, dtype=t, seed=84)
    P8 = torch.randint(0, 256, (M, N), device=dev(), dtype=torch.uint8, generator=torch.Generator(device=dev()).manual_seed(85))
    res = []
    for v in (4, 1):
        old = L.gemm_variant(v)
        plain, drop, resid, gel, dm, dropres = (torch.zeros(M, N, dtype=t, device=dev()) for _ in range(6))
        C8 = torch.zeros(M, N, dtype=torch.uint8, device=dev())
        L.gemm_nt(A, B, plain, bias=bias)
        L.gemm_nt(A, B, drop, bias=bias, drop_p=0.1, drop_site=3, drop_seed=11)
        L.gemm_nt(A, B, resid, R1=R1)
        L.gemm_nt(A, B, dropres, bias=bias, R1=R1, drop_p=0.1, drop_site=5, drop_seed=13, drop_first=True)
        L.gemm_nt(A, B, gel, bias=bias, C2=C8, act=L.ACT_GELU, c2_deriv='q8')
        L.gemm_nt(A, B, dm, Pre=P8, dact=L.DACT_MUL_Q8)
        L.gemm_variant(old)
        res.append((plain, drop, resid, gel, C8, dm, dropres))
    names = ('plain', 'dropout', 'residual', 'gelu', 'gelu derivative q8', '* derivative q8', 'dropout + residual')
    for nm, a, b in zip(names, res[0], res[1]):
        if a.dtype == torch.uint8:
            assert int((a.int() - b.int()).abs().max()) <= 1, nm
        else:
            close(a, b, t, nm + ': 256-tile vs 128-tile kernel', rtol16=2e-2, atol16=2e-2)
    assert torch.equal(res[0][1] == 0, res[1][1] == 0), 'dropout pattern'
    assert torch.equal(res[0][6] == R1, res[1][6] == R1), 'dropout pattern (dropout + residual form)'
    rows = torch.arange(0, M, 997, device=dev())                  # sampled rows of every panel region, incl. the last tiles
    pre = A[rows].float() @ B.float().t()
    close(res[0][0][rows], pre + bias, t, 'plain vs torch')
    close(res[0][2][rows], pre + R1[rows].float(), t, 'residual vs torch')
    close(res[0][3][rows], torch.nn.functional.gelu(pre + bias), t, 'gelu vs torch')
    close(res[0][5][rows], pre * (P8[rows].float() * L.Q8_STEP - L.Q8_OFF), t, '* derivative vs torch')


# (M / 256, N, K): short-tile heights kp = 1 .. 7 behind one round of full tiles at N = 768, and launches that are ALL short tiles (fewer tiles than CUs)
@pytest.mark.parametrize('ntm,N,K', [(86, 768, 256), (96, 768, 192), (107, 768, 128), (117, 768, 256), (128, 768, 128), (139, 768, 256), (149, 768, 128),
                                     (25, 1024, 256), (9, 1024, 384), (70, 3072, 128)])
def test_gemm256_short_tile_tail(ntm, N, K):
    """a4r_gemm_tail_plan: the rows behind the last whole round of 256-row tiles run as short tiles (32 kp rows) in the same launch.  Every
    epilogue form of the training step on full AND short tiles against the 128-tile kernel (same epilogue code, other tiling) and fp32 torch;
    dropout masks identical; the tile-native 8-bit derivative written and read through short tiles equals the row-major pipeline bit for bit."""
    from adapter4rec_amd import _lib as L
    t = torch.bfloat16
    M = ntm * 256
    old_max = L.gemm_tail_max(7)              # (the default uses short tiles up to kp = 3 only)
    try:
        _short_tile_tail_case(L, t, M, N, K, ntm)
    finally:
        L.gemm_tail_max(old_max)


def _short_tile_tail_case(L, t, M, N, K, ntm):
    pf, kp = L.gemm_tail_plan(M, N)
    assert kp >= 1 and pf < ntm, (pf, kp)
    A, B = rnd(M, K, dtype=t, seed=81), rnd(N, K, dtype=t, scale=0.05, seed=82)
    bias, R1 = rnd(N, seed=83), rnd(M, N, dtype=t, seed=84)
    P8 = torch.randint(0, 256, (M, N), device=dev(), dtype=torch.uint8, generator=torch.Generator(device=dev()).manual_seed(85))
    res = []
    for v in (4, 1):
        old = L.gemm_variant(v)
        plain, drop, resid, gel, dm, dropres = (torch.full((M, N), 7.0, dtype=t, device=dev()) for _ in range(6))
        C8 = torch.zeros(M, N, dtype=torch.uint8, device=dev())
        L.gemm_nt(A, B, plain, bias=bias)
        L.gemm_nt(A, B, drop, bias=bias, drop_p=0.1, drop_site=3, drop_seed=11)
        L.gemm_nt(A, B, resid, R1=R1)
        L.gemm_nt(A, B, dropres, bias=bias, R1=R1, drop_p=0.1, drop_site=5, drop_seed=13, drop_first=True)
        L.gemm_nt(A, B, gel, bias=bias, C2=C8, act=L.ACT_GELU, c2_deriv='q8')
        L.gemm_nt(A, B, dm, Pre=P8, dact=L.DACT_MUL_Q8)
        L.gemm_variant(old)
        res.append((plain, drop, resid, gel, C8, dm, dropres))
    names = ('plain', 'dropout', 'residual', 'gelu', 'gelu derivative q8', '* derivative q8', 'dropout + residual')
    for nm, a, b in zip(names, res[0], res[1]):
        if a.dtype == torch.uint8:
            assert int((a.int() - b.int()).abs().max()) <= 1, nm
        else:
            close(a, b, t, nm + ': 256-tile (short tail) vs 128-tile kernel', rtol16=2e-2, atol16=2e-2)
    assert torch.equal(res[0][1] == 0, res[1][1] == 0), 'dropout pattern'
    assert torch.equal(res[0][6] == R1, res[1][6] == R1), 'dropout pattern (dropout + residual form)'
    rows = torch.cat([torch.arange(0, M, 509, device=dev()), torch.arange(pf * 256, M, 37, device=dev())])     # the tail densely
    pre = A[rows].float() @ B.float().t()
    close(res[0][0][rows], pre + bias, t, 'plain vs torch')
    close(res[0][2][rows], pre + R1[rows].float(), t, 'residual vs torch')
    close(res[0][3][rows], torch.nn.functional.gelu(pre + bias), t, 'gelu vs torch')
    close(res[0][5][rows], pre * (P8[rows].float() * L.Q8_STEP - L.Q8_OFF), t, '* derivative vs torch')
    # tile-native derivative through the short tiles
    old = L.gemm_variant(4)
    outs = {}
    for tiled in (False, True):
        Cg = torch.zeros(M, N, dtype=t, device=dev())
        D = torch.zeros(M, N, dtype=torch.uint8, device=dev())
        L.gemm_nt(A, B, Cg, bias=bias, C2=D, act=L.ACT_GELU, c2_deriv='q8', q8_tiled=tiled)
        G = torch.zeros(M, N, dtype=t, device=dev())
        L.gemm_nt(A, B, G, Pre=D, dact=L.DACT_MUL_Q8, q8_tiled=tiled)
        outs[tiled] = (Cg, D, G)
    L.gemm_variant(old)
    assert torch.equal(outs[False][0], outs[True][0]) and torch.equal(outs[False][2], outs[True][2])
    assert torch.equal(outs[False][0], res[0][3])
    assert torch.equal(torch.sort(outs[False][1].flatten())[0], torch.sort(outs[True][1].flatten())[0])
    # fp32 instantiation (the evaluation sweep), plain form
    Af, Bf = A.float(), B.float()
    Cf = torch.zeros(M, N, device=dev())
    old = L.gemm_variant(4)
    L.gemm_nt(Af, Bf, Cf, bias=bias)
    L.gemm_variant(old)
    close(Cf[rows], pre + bias, torch.float32, 'fp32 plain vs torch')


def test_gemm_tail_plan_properties():
    """The split is a function of (M, N) only, keeps at most one short tile per CU and never more full tiles per CU than whole rounds."""
    from adapter4rec_amd import _lib as L
    ncu = 256
    assert (L.gemm_tail_max(-1) != 3 or L.gemm_tail_plan(40448, 768) == (158, 0)) and L.gemm_tail_plan(66304, 768) == (256, 1)
    old_max = L.gemm_tail_max(7)
    plans = {(M, N): L.gemm_tail_plan(M, N) for M, N in [(40448, 768), (40448, 2304), (40448, 3072), (66304, 768), (16896, 3072), (256, 256), (256 * 57, 1024), (160 * 256, 768)]}
    L.gemm_tail_max(old_max)
    assert plans[(40448, 768)] == (85, 7) and plans[(40448, 3072)] == (149, 4)
    for (M, N), (pf, kp) in plans.items():
        ntm, ntn = M // 256, N // 256
        assert 0 <= pf <= ntm and 0 <= kp <= 7
        if kp:
            rows = (ntm - pf) * 256
            assert -(-rows // (32 * kp)) * ntn <= ncu and pf * ntn <= (ntm * ntn // ncu) * ncu
        else:
            assert pf == ntm


# ------------------------------------------------------------------ round 3: e4m3 GEMM outputs, the fused SASRec block
@pytest.mark.parametrize('M,N,K', [(512, 3072, 768), (256 * 5, 1024, 256)])
def test_gemm_fp8_output_static_scale(M, N, K):
    """c_fp8 = 1 (the fp8 encoder's FFN-up): C = e4m3(gelu(.) / c_scale) next to the 8-bit derivative output; the stored bytes are the
    correctly rounded e4m3 of the fp32 epilogue value of the dequantised product."""
    from adapter4rec_amd import _lib as L
    A, B = rnd(M, K, seed=M + 1), rnd(N, K, scale=0.05, seed=N + 2)
    Aq, As = _q8_ref(A)
    Bq, Bs = L.quantize_weight_fp8(B)
    bias = rnd(N, seed=13) * 0.1
    C8 = torch.zeros(M, N, dtype=torch.uint8, device=dev())
    D8 = torch.zeros(M, N, dtype=torch.uint8, device=dev())
    L.gemm_nt(Aq.view(torch.uint8), Bq, C8, bias=bias, C2=D8, act=L.ACT_GELU, c2_deriv='q8', scale_a=As, scale_b=Bs, c_fp8=1, c_scale=0.25)
    pre = (Aq.float() * As[:, None]) @ (Bq.view(torch.float8_e4m3fn).float() * Bs[:, None]).t() + bias
    ref = torch.nn.functional.gelu(pre)
    got = C8.view(torch.float8_e4m3fn).float() * 0.25
    # one e4m3 rounding (2^-4 relative, half a subnormal step 2^-10 * 0.25 absolute) on top of fp32 accumulation-order noise
    err = (got - ref).abs()
    assert bool((err <= 2 ** -4 * ref.abs() + 2 ** -10 * 0.25 + 1e-4).all()), float(err.max())
    want = (ref / 0.25).clamp(-448, 448).to(torch.float8_e4m3fn).view(torch.uint8)
    assert float((C8 != want).float().mean()) < 2e-3            # identical bytes except where accumulation order moves a value across a rounding boundary
    dref = (pre.clone().requires_grad_(True))
    torch.nn.functional.gelu(dref).sum().backward()
    assert float(((D8.float() * L.Q8_STEP - L.Q8_OFF) - dref.grad).abs().max()) < 4e-3


def test_gemm_fp8_output_row_scale_chain():
    """c_fp8 = 2 (the fp8 encoder's FFN dgrads): du = (dy W2) * gelu' leaves as e4m3 with scale_a[m] * c_scale per row, that scale is written
    out, and the next GEMM consumes both: the chain reproduces the fp32 chain to e4m3 rounding."""
    from adapter4rec_amd import _lib as L
    M, H, F = 768, 256, 1024
    dy = rnd(M, H, seed=5) * torch.logspace(-6, -2, M, device=dev())[:, None]          # gradient rows of very different magnitude
    W2, W1 = rnd(H, F, scale=0.03, seed=6), rnd(F, H, scale=0.03, seed=7)              # forward weights [out, in]
    g = torch.rand(M, F, device=dev())                                                  # saved gelu' in [0, 1]
    P8 = torch.clamp(torch.round((g + L.Q8_OFF) / L.Q8_STEP), 0, 255).to(torch.uint8)
    gq = P8.float() * L.Q8_STEP - L.Q8_OFF
    dq, ds = torch.zeros(M, H, dtype=torch.uint8, device=dev()), torch.zeros(M, 1, device=dev())
    L.quant_rows_fp8(dy.to(torch.bfloat16), dq, ds)
    W2T8, W2T8s = L.quantize_weight_fp8(W2.t().contiguous())                            # [F, H]
    W1T8, W1T8s = L.quantize_weight_fp8(W1.t().contiguous())                            # [H, F]
    c_du = 16.0 * float(W2.t().norm(dim=1).max())
    du8, dus = torch.zeros(M, F, dtype=torch.uint8, device=dev()), torch.zeros(M, 1, device=dev())
    L.gemm_nt(dq, W2T8, du8, Pre=P8, dact=L.DACT_MUL_Q8, scale_a=ds, scale_b=W2T8s, c_fp8=2, c_scale=c_du, c_scale_out=dus)
    torch.testing.assert_close(dus, ds * c_du, rtol=1e-6, atol=0)
    dyd = dq.view(torch.float8_e4m3fn).float() * ds
    du_ref = (dyd @ (W2T8.view(torch.float8_e4m3fn).float() * W2T8s[:, None]).t()) * gq
    du_got = du8.view(torch.float8_e4m3fn).float() * dus
    rel = (du_got - du_ref).abs() / du_ref.abs().amax(1, keepdim=True)
    assert float(rel.max()) < 2 ** -4 and float((du8.view(torch.float8_e4m3fn).float().abs() >= 448).float().mean()) == 0.0      # no saturation
    dx = torch.zeros(M, H, dtype=torch.bfloat16, device=dev())
    L.gemm_nt(du8, W1T8, dx, scale_a=dus, scale_b=W1T8s)
    full = ((dy.to(torch.bfloat16).float() @ W2) * g) @ W1                              # the unquantised chain
    err = (dx.float() - full).abs().amax(1) / full.abs().amax(1)
    # per ROW (the row scales carry 4 decades of magnitude): five e4m3 / 8-bit roundings along the chain and a contraction of only 256 / 1 024
    # terms -- measured worst row 0.09, mean 0.05 of the row's maximum
    assert float(err.max()) < 0.15 and float(err.mean()) < 0.08, (float(err.max()), float(err.mean()))


def _sasrec_case(d, act, inner, seed, B=6, T=20, mode=0):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s, sc=1.0: (torch.randn(*s, generator=g) * sc).to(dev())
    desc = dict(wqkv=r(192, 64, sc=0.15), wfc=r(64, 64, sc=0.15), w1=r(256, 64, sc=0.15), b1=r(256, sc=0.1), w2=r(64, 256, sc=0.08), b2=r(64, sc=0.1),
                ln1_g=1 + r(64, sc=0.1), ln1_b=r(64, sc=0.1), ln2_g=1 + r(64, sc=0.1), ln2_b=r(64, sc=0.1),
                E=64, n_heads=2, F=256, d=d, ldwu=64, ldg_d=64, ldg_u=64, act=act, inner_res=int(inner), eps=1e-6, mask_neg=-1e9,
                drop_attn=0.0, drop_hidden=0.0, drop_site=4096, drop_seed=1234567)
    for k in ('1', '2'):
        wd, wu, bd = torch.zeros(64, 64, device=dev()), torch.zeros(64, 64, device=dev()), torch.zeros(64, device=dev())
        wd[:d], wu[:, :d], bd[:d] = r(d, 64, sc=0.2), r(64, d, sc=0.2), r(d, sc=0.1)
        desc.update({'wd' + k: wd, 'bd' + k: bd, 'wu' + k: wu, 'bu' + k: r(64, sc=0.1)})
        desc.update({'g_wd' + k: torch.zeros(64, 64, device=dev()), 'g_wu' + k: torch.zeros(64, 64, device=dev()),
                     'g_bd' + k: torch.zeros(64, device=dev()), 'g_bu' + k: torch.zeros(64, device=dev())})
    if mode == 1:                                                # Pfeiffer form: a third, trainable LayerNorm
        desc.update(mode=1, ln3_g=1 + r(64, sc=0.1), ln3_b=r(64, sc=0.1), g_ln3_g=torch.zeros(64, device=dev()), g_ln3_b=torch.zeros(64, device=dev()))
    x = r(B * T, 64)
    mask = torch.ones(B, T, device=dev())
    for u, pad in enumerate((0, 11, 19, 5, 0, 17)[:B]):
        mask[u, :pad] = 0                                          # left-padded histories (a fully padded query row attends uniformly)
    return desc, x, mask, r(B * T, 64)


@pytest.mark.parametrize('d,act,inner,mode', [(16, 1, True, 0), (16, 3, False, 0), (24, 2, True, 0), (32, 1, True, 0), (16, 1, False, 1), (16, 4, False, 1)])
def test_sasrec_block_vs_torch(d, act, inner, mode):
    """a4r_sasrec_block_fwd / _bwd (one launch per block) vs the same block in torch autograd (tests/sim_lib.py restates
    modules.py:45-87 + model.py:341-376): output, input gradient and the eight adapter gradients, fp32."""
    import sim_lib
    from adapter4rec_amd import _lib as L
    B, T = 6, 20
    desc, x, mask, dy = _sasrec_case(d, act, inner, seed=40 + d + act, mode=mode)
    y = torch.zeros_like(x)
    L.sasrec_block(desc, x, mask, y, B, T, False)
    cpu = lambda t: t.detach().cpu() if torch.is_tensor(t) else t
    dc = {k: cpu(v) for k, v in desc.items()}
    for k in list(dc):
        if k.startswith('g_'):
            dc[k] = torch.zeros_like(dc[k])
    y_ref = torch.zeros(B * T, 64)
    sim_lib.sasrec_block(dc, cpu(x), cpu(mask), y_ref, B, T, False)
    close(y, y_ref, torch.float32, 'sasrec block forward', atol32=5e-5, rtol32=5e-5)
    dx, dx_ref = torch.zeros_like(x), torch.zeros(B * T, 64)
    L.sasrec_block(desc, x, mask, dx, B, T, False, dy=dy)
    sim_lib.sasrec_block(dc, cpu(x), cpu(mask), dx_ref, B, T, False, dy=cpu(dy))
    close(dx, dx_ref, torch.float32, 'sasrec block dx', atol32=1e-4, rtol32=1e-4)
    for k in (('wd2', 'bd2', 'wu2', 'bu2', 'ln3_g', 'ln3_b') if mode == 1 else ('wd1', 'bd1', 'wu1', 'bu1', 'wd2', 'bd2', 'wu2', 'bu2')):
        ref = dc['g_' + k]
        close(desc['g_' + k], ref, torch.float32, 'sasrec block g_' + k, atol32=1e-4 * float(ref.abs().max()) + 1e-6, rtol32=1e-4)
        if k.startswith('wd'):
            assert float(desc['g_' + k][d:].abs().max()) == 0.0           # nothing lands in the zero padding
        if k.startswith('wu'):
            assert float(desc['g_' + k][:, d:].abs().max()) == 0.0


@pytest.mark.parametrize('mode', [0, 1])
def test_sasrec_block_dropout_is_consistent(mode):
    """train = 1: the masks are a pure function of (seed, site, element) -- two forwards agree bit for bit, another seed differs, and the
    backward differentiates the forward WITH its masks (directional derivative of the kernel's own forward)."""
    from adapter4rec_amd import _lib as L
    B, T = 6, 20
    desc, x, mask, dy = _sasrec_case(16, 1, mode == 0, seed=77, mode=mode)
    desc.update(drop_attn=0.1, drop_hidden=0.1)
    y0, y1, y2 = (torch.zeros_like(x) for _ in range(3))
    L.sasrec_block(desc, x, mask, y0, B, T, True)
    L.sasrec_block(desc, x, mask, y1, B, T, True)
    assert torch.equal(y0, y1)
    L.sasrec_block(dict(desc, drop_seed=99), x, mask, y2, B, T, True)
    assert float((y0 - y2).abs().max()) > 1e-3
    ye = torch.zeros_like(x)
    L.sasrec_block(desc, x, mask, ye, B, T, False)
    assert float((y0 - ye).abs().max()) > 1e-3                             # train mode really drops
    v = torch.randn(x.shape, device=x.device, generator=torch.Generator(device=x.device).manual_seed(4242))      # (was unseeded: the verdict depended on the tests that ran before)
    eps = 2e-3

    def fd_check(dd, train, what):
        dx = torch.zeros_like(x)
        L.sasrec_block(dd, x, mask, dx, B, T, train, dy=dy)
        yp, ym = torch.zeros_like(x), torch.zeros_like(x)
        L.sasrec_block(dd, x + eps * v, mask, yp, B, T, train)
        L.sasrec_block(dd, x - eps * v, mask, ym, B, T, train)
        num = float((((yp - ym).double() / (2 * eps)) * dy.double()).sum())
        ana = float((dx.double() * v.double()).sum())
        mag = float((dx.double() * v.double()).abs().sum())                # the sum's natural scale: its terms cancel to a few per cent of this
        print(f'{what}: directional derivative numeric {num:.4f} analytic {ana:.4f} (sum of |terms| {mag:.1f})')
        return num, ana, mag
    n0, a0, m0 = fd_check(desc, False, 'no dropout')                       # calibrates the method (fp32 central difference through LN / softmax / ReLU kinks)
    rel0 = abs(n0 - a0) / m0
    for dd, what in ((dict(desc, drop_hidden=0.0), 'attention dropout only'), (dict(desc, drop_attn=0.0), 'hidden dropout only'), (desc, 'both')):
        num, ana, mag = fd_check(dd, True, what)
        assert abs(num - ana) / mag < max(3.0 * rel0, 2e-2), (what, num, ana, mag, rel0)


# 160 tiles: the 256-tile kernel alone (fewer than 128 tiles go to the 128-tile kernel, row-major either way); 264 tiles: one round + a tail
# row-panel pair on the 128-tile kernel, whose rows stay row-major
@pytest.mark.parametrize('M,N,K', [(256 * 40, 1024, 256), (256 * 66, 1024, 128)])
def test_gemm_q8_tiled_layout_roundtrip(M, N, K):
    """a4r_gemm_t.q8_tiled: the 8-bit GELU derivative written by the FFN-up launch in the 256-tile kernel's own order and read back by the
    `* derivative` dgrad launch gives bit-identical results to the row-major pipeline; the stored bytes are a permutation of the row-major ones."""
    from adapter4rec_amd import _lib as L
    t = torch.bfloat16
    A, B = rnd(M, K, dtype=t, seed=1), rnd(N, K, dtype=t, scale=0.1, seed=2)
    dY, W = rnd(M, K, dtype=t, seed=3), rnd(N, K, dtype=t, scale=0.1, seed=4)
    bias = rnd(N, seed=5) * 0.1
    outs = {}
    for tiled in (False, True):
        C = torch.zeros(M, N, dtype=t, device=dev())
        D = torch.zeros(M, N, dtype=torch.uint8, device=dev())
        L.gemm_nt(A, B, C, bias=bias, C2=D, act=L.ACT_GELU, c2_deriv='q8', q8_tiled=tiled)
        G = torch.zeros(M, N, dtype=t, device=dev())
        L.gemm_nt(dY, W, G, Pre=D, dact=L.DACT_MUL_Q8, q8_tiled=tiled)
        outs[tiled] = (C, D, G)
    assert torch.equal(outs[False][0], outs[True][0]) and torch.equal(outs[False][2], outs[True][2])
    d0, d1 = outs[False][1], outs[True][1]
    assert not torch.equal(d0, d1) and torch.equal(torch.sort(d0.flatten())[0], torch.sort(d1.flatten())[0])
    # a tile's bytes hold exactly that tile's values: a full tile (65 536 bytes at tile index * 65 536), and a short tile of the tail
    # (a4r_gemm_tail_plan: row panel at row r0 starts at byte r0 * N; its N-tiles of 32 kp x 256 bytes follow each other)
    pf, kp = L.gemm_tail_plan(M, N)
    tn = 2
    if pf > 1:
        tm = 1
        tile_rm = d0[tm * 256:(tm + 1) * 256, tn * 256:(tn + 1) * 256].flatten()
        tile_t = d1.flatten()[(tm * (N // 256) + tn) * 65536:(tm * (N // 256) + tn + 1) * 65536]
        assert torch.equal(torch.sort(tile_rm)[0], torch.sort(tile_t)[0])
    if kp:
        h = 32 * kp
        r0 = pf * 256 + h                                   # the second short row panel
        tile_rm = d0[r0:r0 + h, tn * 256:(tn + 1) * 256].flatten()
        tile_t = d1.flatten()[r0 * N + tn * h * 256:r0 * N + (tn + 1) * h * 256]
        assert torch.equal(torch.sort(tile_rm)[0], torch.sort(tile_t)[0])


# an e4m3 FFN-up launch (always the 256-tile kernel) writes the tile-native derivative that a bf16 dgrad launch reads -- at a shape
# the bf16 launch gives to the 128-tile kernel (16 tiles) and at one whose last row panels it hands over (264 tiles, short tiles switched off)
@pytest.mark.parametrize('M,N,K,tail', [(1024, 1024, 256, None), (256 * 66, 1024, 128, 0), (256 * 66, 1024, 128, None)])
def test_gemm_q8_tiled_fp8_writer_bf16_reader(M, N, K, tail):
    """The layout of a q8_tiled tensor is a function of (M, N) only (a4r_gemm_rows_256): an e4m3 writer and a bf16 reader (and the reverse
    pair) of the same [M, N] agree on it, so the tiled pipeline equals the row-major one bit for bit."""
    from adapter4rec_amd import _lib as L
    t = torch.bfloat16
    old = L.gemm_tail_max(tail) if tail is not None else None
    try:
        rows = L.gemm_rows_256(M, N)
        assert rows % 256 == 0 and 0 <= rows <= M
        if (M, tail) == (1024, None):
            assert rows == 0
        if tail == 0:
            assert 0 < rows < M
        A, B = rnd(M, K, dtype=t, seed=1), rnd(N, K, dtype=t, scale=0.1, seed=2)
        dY, W = rnd(M, K, dtype=t, seed=3), rnd(N, K, dtype=t, scale=0.1, seed=4)
        bias = rnd(N, seed=5) * 0.1
        A8, As = torch.zeros(M, K, dtype=torch.uint8, device=dev()), torch.zeros(M, 1, device=dev())
        L.quant_rows_fp8(A, A8, As)
        B8, Bs = L.quantize_weight_fp8(B)
        dY8, dYs = torch.zeros(M, K, dtype=torch.uint8, device=dev()), torch.zeros(M, 1, device=dev())
        L.quant_rows_fp8(dY, dY8, dYs)
        W8, Ws = L.quantize_weight_fp8(W)
        outs = {}
        for tiled in (False, True):
            C = torch.zeros(M, N, dtype=t, device=dev())
            D = torch.zeros(M, N, dtype=torch.uint8, device=dev())
            L.gemm_nt(A8, B8, C, bias=bias, C2=D, act=L.ACT_GELU, c2_deriv='q8', scale_a=As, scale_b=Bs, q8_tiled=tiled)       # e4m3 writer
            G = torch.zeros(M, N, dtype=t, device=dev())
            L.gemm_nt(dY, W, G, Pre=D, dact=L.DACT_MUL_Q8, q8_tiled=tiled)                                                    # bf16 reader
            D2 = torch.zeros(M, N, dtype=torch.uint8, device=dev())
            C2_ = torch.zeros(M, N, dtype=t, device=dev())
            L.gemm_nt(A, B, C2_, bias=bias, C2=D2, act=L.ACT_GELU, c2_deriv='q8', q8_tiled=tiled)                              # bf16 writer
            G8 = torch.zeros(M, N, dtype=torch.uint8, device=dev())
            G8s = torch.zeros(M, 1, device=dev())
            L.gemm_nt(dY8, W8, G8, Pre=D2, dact=L.DACT_MUL_Q8, scale_a=dYs, scale_b=Ws, c_fp8=2, c_scale=2.0, c_scale_out=G8s,
                      q8_tiled=tiled)                                                                                          # e4m3 reader
            outs[tiled] = (C, G, G8, G8s, D)
        for i in range(4):
            assert torch.equal(outs[False][i], outs[True][i]), i
        d0, d1 = outs[False][4], outs[True][4]
        assert torch.equal(d0[rows:], d1[rows:])                   # row-major behind the 256-tile rows
        if rows:
            assert not torch.equal(d0[:rows], d1[:rows]) and torch.equal(torch.sort(d0[:rows].flatten())[0], torch.sort(d1[:rows].flatten())[0])
    finally:
        if old is not None:
            L.gemm_tail_max(old)


@pytest.mark.parametrize('H', [256, 768])
@pytest.mark.parametrize('act,inner,sums,drop', [(1, True, 'b', 0.1), (3, False, '', 0.0)])
def test_adapter_ln_bwd_from_y(H, act, inner, sums, drop):
    """beta_y: the forward kept only y = LN(v) (a4r_adapter_ln_fwd with v = NULL) and the backward rebuilds xhat = (y - beta) / gamma.
    Against the v-based launch on the same sub-layer: xhat differs by y's bf16 rounding only."""
    from adapter4rec_amd import _lib as L
    M, Mp, dp, t = 16 * 301, 16 * 304, 64, torch.bfloat16
    A, R, Wd, Wu, bd, bu, gamma, beta = _adapter_case(H, Mp, seed=220)
    mk = lambda c: torch.zeros(Mp, c, dtype=t, device=dev())
    zp, z, v, y, y_only = mk(dp), mk(dp), mk(H), mk(H), mk(H)
    st, st2 = torch.zeros(Mp, 2, device=dev()), torch.zeros(Mp, 2, device=dev())
    r1, r2 = (A, R) if inner else (R, None)
    L.adapter_ln_fwd(A, r1, r2, Wd, bd, Wu, bu, gamma, beta, 1e-12, act, zp, z, v, y, st, M=M)
    zp2, z2 = mk(dp), mk(dp)
    L.adapter_ln_fwd(A, r1, r2, Wd, bd, Wu, bu, gamma, beta, 1e-12, act, zp2, z2, None, y_only, st2, M=M)        # v not stored
    assert torch.equal(y, y_only) and torch.equal(st, st2) and torch.equal(zp, zp2)
    dy = rnd(Mp, H, dtype=t, seed=231)
    WuT, WdT = Wu.t().contiguous(), Wd.t().contiguous()
    outs = []
    for src, by in ((v, None), (y, beta)):
        dv, dzp, dh = mk(H), mk(dp), mk(H)
        dbi = torch.zeros(H, device=dev()) if 'b' in sums else None
        dbd = torch.zeros(dp, device=dev()) if 'b' in sums else None
        L.adapter_ln_bwd(dy, src, st, gamma, None, zp, act, WuT, WdT, inner, dv, dzp, dh, dbias=dbi, M=M, drop_p=drop, drop_site=9, drop_seed=4242,
                         dbd=dbd, beta_y=by)
        outs.append((dv, dzp, dh, dbi, dbd))
    (dv0, dz0, dh0, b0, d0), (dv1, dz1, dh1, b1, d1) = outs
    # torch fp32 from the UNROUNDED LayerNorm input is the common reference: both launches sit within bf16 rounding of it
    vf = v.float()[:M]
    mean, rstd = st[:M, 0:1], st[:M, 1:2]
    xh = (vf - mean) * rstd
    gq = dy[:M].float() * gamma
    dv_r = rstd * (gq - gq.mean(-1, keepdim=True) - xh * (gq * xh).mean(-1, keepdim=True))
    e0, e1 = float((dv0[:M].float() - dv_r).abs().max()), float((dv1[:M].float() - dv_r).abs().max())
    scale = float(dv_r.abs().max())
    print(f'H={H}: dv error vs fp32 torch: from v {e0 / scale:.2e}, from y {e1 / scale:.2e} (of max |dv| {scale:.3f})')
    assert e1 < 3.0 * e0 + 2e-2 * scale
    close(dv1[:M], dv0[:M], t, 'dv from y vs from v', rtol16=3e-2, atol16=2e-2 * scale)
    close(dz1[:M], dz0[:M], t, 'dzp from y vs from v', rtol16=5e-2, atol16=3e-2 * float(dz0.float().abs().max()))
    if drop:
        assert torch.equal(dh0[:M] == 0, dh1[:M] == 0)
    close(dh1[:M], dh0[:M], t, 'dh from y vs from v', rtol16=5e-2, atol16=3e-2 * float(dh0.float().abs().max()))
    if b0 is not None:
        close(b1, b0, torch.float32, 'dbias', atol32=3e-2 * max(1.0, float(b0.abs().max())), rtol32=3e-2)
        close(d1, d0, torch.float32, 'dbd', atol32=3e-2 * max(1.0, float(d0.abs().max())), rtol32=3e-2)


@pytest.mark.parametrize('n_items,NP,n_keep', [(84, 196, 49), (7, 16, 4), (3, 1000, 1000)])
def test_mae_keep_indices(n_items, NP, n_keep):
    """a4r_mae_keep_indices (HF ViTMAEEmbeddings.random_masking under Downstream/CV/model/encoders.py:8-22): explicit noise -> bit-equal to
    a stable argsort, ties included; noise drawn on the device -> distinct in-range indices per item, reproducible per seed, uniform."""
    from adapter4rec_amd import _lib as L
    g = torch.Generator().manual_seed(3)
    noise = torch.rand(n_items, NP, generator=g)
    noise[0, : NP // 2] = noise[0, NP // 2: 2 * (NP // 2)]            # ties: the stable order decides
    noise[-1] = 0.25
    keep = torch.full((n_items, n_keep), -1, dtype=torch.int32, device=dev())
    L.mae_keep_indices(keep, NP, noise.to(dev()))
    ref = torch.argsort(noise, dim=1, stable=True)[:, :n_keep].to(torch.int32)
    assert torch.equal(keep.cpu(), ref)
    k1 = torch.full((n_items, n_keep), -1, dtype=torch.int32, device=dev())
    k2, k3 = k1.clone(), k1.clone()
    L.mae_keep_indices(k1, NP, None, seed=77, site=4900)
    L.mae_keep_indices(k2, NP, None, seed=77, site=4900)
    L.mae_keep_indices(k3, NP, None, seed=78, site=4900)
    assert torch.equal(k1, k2) and (n_keep == NP or not torch.equal(k1, k3))
    srt = torch.sort(k1.long(), dim=1)[0]
    assert int(srt.min()) >= 0 and int(srt.max()) < NP and bool((srt[:, 1:] > srt[:, :-1]).all())


def test_mae_keep_indices_uniform():
    from adapter4rec_amd import _lib as L
    n_items, NP, n_keep = 4096, 196, 49
    k = torch.zeros(n_items, n_keep, dtype=torch.int32, device=dev())
    L.mae_keep_indices(k, NP, None, seed=5, site=4900)
    cnt = torch.bincount(k.flatten().long().cpu(), minlength=NP).double()
    p = n_keep / NP
    z = (cnt - n_items * p) / (n_items * p * (1 - p)) ** 0.5
    assert float(z.abs().max()) < 5.0, float(z.abs().max())
    first = torch.bincount(k[:, 0].long().cpu(), minlength=NP).double()        # the smallest-noise patch is uniform over the patches
    z0 = (first - n_items / NP) / (n_items / NP) ** 0.5
    assert float(z0.abs().max()) < 5.0, float(z0.abs().max())


@pytest.mark.parametrize('M,N,K', [(40448, 768, 3072), (40448, 3072, 768), (16896, 2304, 768), (40448, 768, 192), (2560, 768, 2304)])
def test_gemm256_ring_race_screen(M, N, K):
    """The LDS-DMA ring of the 256-tile kernel (two phases per K-tile since round 4: fragment reads retired in front of the barrier that ends
    a LOAD segment, A_hi re-filled one interval after its last read): the launch is deterministic, so a run that differs bitwise from the first
    is a fragment read that overtook its DMA or a slot re-filled under a reader.  Twelve runs per shape, every other one beside 512 MB of
    copy traffic on a second stream (moves the DMA landing times); even and odd K-tile counts, short-tile tails, a banded map.
    tools/gemm_race_screen.py is the long form (more shapes, fp32, the epilogue forms of the step)."""
    from adapter4rec_amd import _lib as L
    t = torch.bfloat16
    A, B = rnd(M, K, dtype=t, seed=1), rnd(N, K, dtype=t, scale=0.05, seed=2)
    bias = rnd(N, seed=3) * 0.1
    side = torch.cuda.Stream()
    ja, jb = torch.empty(64 << 20, device=dev()), torch.empty(64 << 20, device=dev())
    first = None
    for it in range(12):
        C = torch.empty(M, N, dtype=t, device=dev())
        if it % 2:
            with torch.cuda.stream(side):
                jb.copy_(ja)
        L.gemm_nt(A, B, C, bias=bias)
        torch.cuda.synchronize()
        if first is None:
            first = C
            ref = A.float() @ B.float().t() + bias
            assert float((C.float() - ref).abs().max() / ref.abs().max()) < 2e-2
        else:
            assert torch.equal(C, first), f'run {it} differs from run 0'


@pytest.mark.parametrize('t', [torch.bfloat16, torch.float32])
@pytest.mark.parametrize('twin', [True, False])
def test_ln_fwd_sum(t, twin):
    """a4r_ln_fwd_sum: y = LN(h + residual), sum in fp32, normalised unrounded; residual = the fp32 twin or the T tensor; outputs sum (T),
    sum32, y32, stats -- against torch fp32."""
    from adapter4rec_amd import _lib as L
    M, H = 16 * 301, 768
    h, r = rnd(M, H, dtype=t, seed=1), rnd(M, H, dtype=t, seed=2) * 3.0
    r32 = rnd(M, H, seed=3) * 3.0
    gamma, beta = 1.0 + 0.1 * rnd(H, seed=4), 0.1 * rnd(H, seed=5)
    y, sm = torch.zeros(M, H, dtype=t, device=dev()), torch.zeros(M, H, dtype=t, device=dev())
    s32, y32, st = torch.zeros(M, H, device=dev()), torch.zeros(M, H, device=dev()), torch.zeros(M, 2, device=dev())
    L.ln_fwd_sum(h, r, gamma, beta, 1e-12, y, st, res32=r32 if twin else None, sum_out=sm, sum32=s32, y32=y32)
    ref_s = h.float() + (r32 if twin else r.float())
    ref_y = torch.nn.functional.layer_norm(ref_s, (H,), gamma, beta, 1e-12)
    close(s32, ref_s, torch.float32, 'sum32', atol32=1e-6, rtol32=1e-6)
    close(sm, ref_s, t, 'sum')
    close(y32, ref_y, torch.float32, 'y32', atol32=2e-5, rtol32=2e-5)
    close(y, ref_y, t, 'y')
    close(st[:, 0], ref_s.mean(-1), torch.float32, 'mean', atol32=1e-5, rtol32=1e-5)
    close(st[:, 1], torch.rsqrt(ref_s.var(-1, unbiased=False) + 1e-12), torch.float32, 'rstd', atol32=1e-5, rtol32=1e-4)
    y2, st2 = torch.zeros(M, H, dtype=t, device=dev()), torch.zeros(M, 2, device=dev())
    L.ln_fwd_sum(h, r, gamma, beta, 1e-12, y2, st2, res32=r32 if twin else None)          # the optional outputs do not change y
    assert torch.equal(y, y2) and torch.equal(st, st2)


@pytest.mark.parametrize('H', [128, 256, 512, 768])
def test_adapter_ln_fragment_ordered_weights_bit_equal(H):
    """ABI 408: the one-launch adapter kernels read their two weight matrices in FRAGMENT order (a4r_pack_matrices layouts 1 / 2: 1 KiB contiguous
    per wave instruction in the prologue).  Same values, same arithmetic: every output bit-equal to the row-major launch; the copies come from
    a4r_pack_matrices itself (fp32 masters -> bf16, with and without the transpose), so the pack kernel's index formulas are under test too."""
    import ctypes as C
    from adapter4rec_amd import _lib as L
    M, dp, d, t = 16 * 37, 64, 48, torch.bfloat16                      # bottleneck 48, padded to 64 by the pack
    A, R, _, _, bd, bu, gamma, beta = _adapter_case(H, M, seed=300 + H)
    g = torch.Generator(device='cpu').manual_seed(H)
    wd32 = (torch.randn(d, H, generator=g) * 0.05).to(dev())           # fc_down.weight [d, H], fc_up.weight [H, d]: the fp32 masters
    wu32 = (torch.randn(H, d, generator=g) * 0.05).to(dev())
    flat = torch.cat([wd32.reshape(-1), wu32.reshape(-1)])
    o_wd, o_wu = 0, d * H
    mkw = lambda r, c: torch.zeros(r, c, dtype=t, device=dev())
    Wd, Wu, WuT, WdT = mkw(dp, H), mkw(H, dp), mkw(dp, H), mkw(H, dp)
    f_wd, f_wu, f_wuT, f_wdT = mkw(dp, H), mkw(H, dp), mkw(dp, H), mkw(H, dp)       # fragment-ordered twins (viewed with their logical shape)
    ents = [(o_wd, Wd, d, H, 0), (o_wu, Wu, H, d, 0), (o_wu, WuT, H, d, 1), (o_wd, WdT, d, H, 1),
            (o_wd, f_wd, d, H, 2), (o_wu, f_wu, H, d, 4), (o_wu, f_wuT, H, d, 2 | 1), (o_wd, f_wdT, d, H, 4 | 1)]
    arr = (L.PackDesc * len(ents))()
    for i, (off, dst, rows, cols, code) in enumerate(ents):
        arr[i] = L.PackDesc(off, dst.data_ptr(), rows, cols, dst.shape[0], dst.shape[1], code, 0)
    tab = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(dev())
    L.pack_matrices(flat, tab, len(ents), dp * H, L.BF16)
    torch.cuda.synchronize()
    assert torch.equal(Wd[:d].float(), wd32.to(t).float()) and torch.equal(WuT[:d].float(), wu32.t().to(t).float())
    assert sorted(f_wd.view(-1).tolist()) == sorted(Wd.view(-1).tolist())            # a permutation of the same values
    mk = lambda c: torch.zeros(M, c, dtype=t, device=dev())
    bdp = torch.zeros(dp, device=dev()); bdp[:d] = bd[:d]
    outs = []
    for frag in (None, (f_wd, f_wu)):
        zp, z, v, y, st = mk(dp), mk(dp), mk(H), mk(H), torch.zeros(M, 2, device=dev())
        L.adapter_ln_fwd(A, A, R, Wd, bdp, Wu, bu, gamma, beta, 1e-12, 1, zp, z, v, y, st, frag=frag)
        outs.append((zp, z, v, y, st))
    for a, b, nm in zip(outs[0], outs[1], ('zp', 'z', 'v', 'y', 'stats')):
        assert torch.equal(a, b), f'forward {nm}: fragment-ordered launch differs'
    assert float(outs[0][1].abs().max()) > 0
    zp, _, v, _, st = outs[0]
    dy = rnd(M, H, dtype=t, seed=41)
    outs = []
    for frag in (None, (f_wuT, f_wdT)):
        dv, dzp, dh, dbi, dbd = mk(H), mk(dp), mk(H), torch.zeros(H, device=dev()), torch.zeros(dp, device=dev())
        L.adapter_ln_bwd(dy, v, st, gamma, None, zp, 1, WuT, WdT, True, dv, dzp, dh, dbias=dbi, drop_p=0.1, drop_site=5, drop_seed=77, dbd=dbd, frag=frag)
        outs.append((dv, dzp, dh))
    for a, b, nm in zip(outs[0], outs[1], ('dv', 'dzp', 'dh')):
        assert torch.equal(a, b), f'backward {nm}: fragment-ordered launch differs'
    assert float(outs[0][2].abs().max()) > 0



def test_adapter_ln_fwd_24bit_residual_stream():
    """--residual_dtype bf24 (ABI 409, w_frag bit 1): the fused adapter forward reads its residual as bf16 tensor + byte plane (a 24-bit float) and writes
    y the same way.  (a) the byte plane it writes joins with y (bf16) to the fp32 LayerNorm output within 2^-16 relative (the fp32 twin of the same
    launch is the reference); (b) fed back as the residual of a second launch, the result equals the launch fed the fp32 twin to 1e-5 -- and differs
    from the launch fed the bf16 tensor alone; (c) the plane is exactly what tests/sim_lib.lo8_of restates."""
    from adapter4rec_amd import _lib as L
    import sim_lib
    M, H, d = 2048, 768, 64
    t = torch.bfloat16
    A, R = rnd(M, H, dtype=t, seed=1), rnd(M, H, dtype=t, seed=2)
    Wd, Wu = rnd(d, H, dtype=t, scale=0.05, seed=3), rnd(H, d, dtype=t, scale=0.05, seed=4)
    bd, bu, gam, bet = rnd(d, scale=0.1, seed=5), rnd(H, scale=0.1, seed=6), 1 + rnd(H, scale=0.1, seed=7), rnd(H, scale=0.1, seed=8)
    mk = lambda c, dt=t: torch.zeros(M, c, dtype=dt, device=dev())
    def run(res=None, twin_dtype=None):
        zp, z, v, y, st = mk(d), mk(d), mk(H), mk(H), torch.zeros(M, 2, device=dev())
        tw = mk(H, twin_dtype) if twin_dtype is not None else None
        L.adapter_ln_fwd(A, A, R, Wd, bd, Wu, bu, gam, bet, 1e-12, L.ACT_GELU, zp, z, v, y, st, **(dict(res32=res, y32=tw) if (res is not None or tw is not None) else {}))
        return y, tw
    y0, y32 = run(twin_dtype=torch.float32)
    y1, y8 = run(twin_dtype=torch.int8)
    assert torch.equal(y0, y1)                                   # the bf16 tensor the GEMMs read is untouched
    joined = sim_lib.lo8_join(y1.cpu(), y8.cpu())
    rel = ((joined - y32.cpu()).abs() / y32.cpu().abs().clamp_min(1e-3)).max().item()
    assert rel < 2.0 ** -14, rel                        # (7 + 8 = 15 explicit mantissa bits, truncated: < 2^-15)
    assert float((y1.float().cpu() - y32.cpu()).abs().max()) > 20 * float((joined - y32.cpu()).abs().max())      # ... and far closer than bf16 alone
    assert torch.equal(y8.cpu(), sim_lib.lo8_of(y32.cpu(), y1.cpu()))             # (both cut the SAME fp32 values: the kernel writes y32 and the plane from one register)
    # second launch: residual = the first launch's output, as fp32 twin / as byte plane / bf16 only
    R2 = y1
    def run2(res):
        zp, z, v, y, st = mk(d), mk(d), mk(H), mk(H), torch.zeros(M, 2, device=dev())
        out32 = mk(H, torch.float32) if (res is None or res.dtype == torch.float32) else None
        o8 = mk(H, torch.int8) if out32 is None else None
        L.adapter_ln_fwd(A, A, R2, Wd, bd, Wu, bu, gam, bet, 1e-12, L.ACT_GELU, zp, z, v, y, st, res32=res, y32=out32 if out32 is not None else o8)
        return out32 if out32 is not None else sim_lib.lo8_join(y.cpu(), o8.cpu()).to(dev())
    f32 = run2(y32)
    b24 = run2(y8)
    b16 = run2(None)
    e24, e16 = float((b24 - f32).abs().max()), float((b16 - f32).abs().max())
    print(f'second sub-layer vs the fp32-stream launch: 24-bit stream {e24:.2e}, bf16 stream {e16:.2e}')
    assert e24 < 2e-4 and e16 > 10 * e24


@pytest.mark.gpu
def test_adapter_ln_fwd_20bit_residual_stream():
    """--residual_dtype bf20 (w_frag bits 1 + 2): the same with a signed NIBBLE per element, rounded to nearest (int8 [M, H / 2], eight elements per 32-bit
    word).  (a) y (bf16) + its nibble plane = the fp32 LayerNorm output within 2^-12 relative (11 explicit mantissa bits, rounded: 2^-13 + the clamp at
    an upward tie); (b) as the residual of a second launch: within 3e-3 of the launch fed the fp32 twin and >= 5 x closer than the bf16 tensor alone;
    (c) the plane is exactly tests/sim_lib.lo4_of; (d) a plane of the wrong width is refused."""
    from adapter4rec_amd import _lib as L
    import sim_lib
    M, H, d = 2048, 768, 64
    t = torch.bfloat16
    A, R = rnd(M, H, dtype=t, seed=1), rnd(M, H, dtype=t, seed=2)
    Wd, Wu = rnd(d, H, dtype=t, scale=0.05, seed=3), rnd(H, d, dtype=t, scale=0.05, seed=4)
    bd, bu, gam, bet = rnd(d, scale=0.1, seed=5), rnd(H, scale=0.1, seed=6), 1 + rnd(H, scale=0.1, seed=7), rnd(H, scale=0.1, seed=8)
    mk = lambda c, dt=t: torch.zeros(M, c, dtype=dt, device=dev())
    def run(resid, res=None, twin=None):
        zp, z, v, y, st = mk(d), mk(d), mk(H), mk(H), torch.zeros(M, 2, device=dev())
        L.adapter_ln_fwd(A, A, resid, Wd, bd, Wu, bu, gam, bet, 1e-12, L.ACT_GELU, zp, z, v, y, st, **(dict(res32=res, y32=twin) if (res is not None or twin is not None) else {}))
        return y
    y32, y4 = mk(H, torch.float32), mk(H // 2, torch.int8)
    y0 = run(R, twin=y32)
    y1 = run(R, twin=y4)
    assert torch.equal(y0, y1)
    joined = sim_lib.lo4_join(y1.cpu(), y4.cpu())
    rel = ((joined - y32.cpu()).abs() / y32.cpu().abs().clamp_min(1e-3)).max().item()
    assert rel < 2.0 ** -11, rel
    assert float((y1.float().cpu() - y32.cpu()).abs().max()) > 4 * float((joined - y32.cpu()).abs().max())
    assert torch.equal(y4.cpu(), sim_lib.lo4_of(y32.cpu(), y1.cpu()))
    o32, o4 = mk(H, torch.float32), mk(H // 2, torch.int8)
    run(y1, res=y32, twin=o32)
    yb = run(y1, res=y4, twin=o4)
    b20 = sim_lib.lo4_join(yb.cpu(), o4.cpu()).to(dev())
    o16 = mk(H, torch.float32)
    run(y1, twin=o16)
    e20, e16 = float((b20 - o32).abs().max()), float((o16 - o32).abs().max())
    print(f'second sub-layer vs the fp32-stream launch: 20-bit stream {e20:.2e}, bf16 stream {e16:.2e}')
    assert e20 < 3e-3 and e16 > 3 * e20
    with pytest.raises((RuntimeError, AssertionError)):
        run(y1, res=mk(H // 4, torch.int8), twin=mk(H // 4, torch.int8))
