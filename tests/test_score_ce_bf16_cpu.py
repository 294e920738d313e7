"""CPU: the bf16 cross-entropy head of the ID tower (--ce_dtype bf16) -- the rounding helper of tests/score_ce_bf16_ref.py pinned to torch's bfloat16,
the derived error bound shown to hold for a numpy emulation of the arithmetic the kernels are allowed on every shape the GPU file uses (so the
reference and its bound are known to be sound before a kernel is held to them), the flag, the refusals, the workspace query, and the C
boundary of the new exports: include/a4r_score_ce_bf16.h against the binding's table (adapter4rec_amd/_lib_ce_bf16.py) and the built library."""
import numpy as np
import pytest
import torch

import score_ce_bf16_ref as B16
import test_id_tower_cpu as CPU
import test_score_ce_gpu as G32

SCALE = 0.37


def test_round_bf16_equals_torch_bit_for_bit():
    rng = np.random.default_rng(0)
    x = np.concatenate([
        rng.standard_normal(4096).astype(np.float32) * np.float32(10.0) ** rng.integers(-6, 7, 4096).astype(np.float32),
        # ties: the 16 dropped bits are exactly 0x8000, after an even and after an odd kept bit, both signs; and just beside a tie
        np.array([0x3f808000, 0x3f818000, 0xbf808000, 0xbf818000, 0x3f807fff, 0x3f808001, 0x7f7f8000, 0x7f7fffff, 0x00008000, 0x00018000],
                 np.uint32).view(np.float32),
        np.array([0x00000001, 0x00007fff, 0x0000ffff, 0x007fffff, 0x807fffff, 0x00800000, 0x00400000], np.uint32).view(np.float32),      # denormals
        np.array([np.inf, -np.inf, 0.0, -0.0, 1.0, -1.0, 3.3895314e38], np.float32)])
    got = B16.round_bf16(x)
    want = torch.from_numpy(x).bfloat16().float().numpy()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert not (got.view(np.uint32) & 0xffff).any()
    assert np.isinf(B16.round_bf16(np.array([3.3961775e38], np.float32))[0])          # above the largest bf16 + half an ulp: rounds to inf
    assert np.isnan(B16.round_bf16(np.array([np.nan], np.float32))[0])
    assert B16.round_bf16(np.zeros((3, 5), np.float32)).shape == (3, 5)


def emulate(prec_b, table_b, tgt, mask, g, round_first):
    """The arithmetic a4r_score_ce_bf16_* may use, in numpy: bf16 operands, fp32 scores and lse, the probability rounded to bf16 before
    (round_first) or after the one-hot is subtracted, both second products accumulated in fp32."""
    f32 = np.float32
    R = prec_b.shape[0]
    s = prec_b @ table_b[1:].T                                              # fp32
    mx = s.max(1)
    lse = (mx + np.log(np.exp(s - mx[:, None]).sum(1, dtype=f32))).astype(f32)
    p = np.exp(s - lse[:, None]).astype(f32)
    trained = (mask != 0) & (tgt != 0)
    count = int(trained.sum())
    gw = f32(g / count) if count else f32(0)
    onehot = np.zeros_like(p)
    has = np.flatnonzero(tgt != 0)
    onehot[has, tgt[has] - 1] = 1
    coef = B16.round_bf16(p) - onehot if round_first else B16.round_bf16(p - onehot)
    coef = (coef * trained[:, None]).astype(f32)
    d_table = np.zeros_like(table_b)
    d_table[1:] = gw * (coef.T @ prec_b)
    return gw * (coef @ table_b[1:]), d_table, lse


ALL_SHAPES = B16.SHAPES + B16.WIDE_SHAPES + [B16.WORKLOAD] + B16.OTHER_SHAPES


@pytest.mark.parametrize('R,N,E,ranges', ALL_SHAPES)
def test_bound_holds_for_the_allowed_arithmetic(R, N, E, ranges):
    case = G32.make_case(R, N, E)
    prec, table, tgt, mask = case
    ref = B16.reference(*case)
    prec_b, table_b = B16.round_bf16(prec), B16.round_bf16(table)
    b_prec, b_table = B16.bounds(ref, prec_b, table_b, tgt, SCALE)
    assert b_prec.shape == prec.shape and b_table.shape == table.shape
    # under 1 % of the gradients' size at every test input with more than one item; with a single item p = 1 and every gradient is exactly 0
    gp, gt = np.abs(ref['d_prec'] * SCALE).max(), np.abs(ref['d_table'] * SCALE).max()
    if N > 1:
        assert b_prec.max() <= 0.01 * gp and b_table.max() <= 0.01 * gt, (b_prec.max() / gp, b_table.max() / gt)
    else:
        assert gp <= 1e-15 and gt <= 1e-15
    for round_first in (True, False):
        d_prec, d_table, lse = emulate(prec_b, table_b, tgt, mask, SCALE, round_first)
        assert np.abs(lse - ref['lse']).max() <= 2e-4
        assert np.all(np.abs(d_prec - ref['d_prec'] * SCALE) <= b_prec)
        assert np.all(np.abs(d_table - ref['d_table'] * SCALE) <= b_table)
    # the bound has teeth: a dropped 16-item tile is outside it (where a tile is more than 2^-8 of the table)
    if ref['count'] and 1 < N <= 257:
        dropped = SCALE * ref['w'][:, None] * (ref['p'][:, :16] @ table_b[1:17].astype(np.float64))
        assert not np.all(np.abs(dropped) <= b_prec)


def test_parser_accepts_ce_dtype_and_defaults_to_fp32():
    from adapter4rec_amd.cv.parameters import parse_args
    assert parse_args([]).ce_dtype == 'fp32'
    assert parse_args(['--loss', 'ce']).ce_dtype == 'fp32'
    assert parse_args(['--loss', 'ce', '--compute_dtype', 'bf16']).ce_dtype == 'fp32'          # --compute_dtype does not imply it
    assert parse_args(['--loss', 'ce', '--ce_dtype', 'bf16']).ce_dtype == 'bf16'
    with pytest.raises(SystemExit):
        parse_args(['--ce_dtype', 'fp16'])


def test_model_keeps_the_flag_and_the_state_dict():
    from adapter4rec_amd.cv import Model
    a, b = Model(CPU.make_args(loss='ce', ce_dtype='bf16'), 60, False), Model(CPU.make_args(loss='ce'), 60, False)
    assert a.ce_dtype == 'bf16' and b.ce_dtype == 'fp32' and a.loss == b.loss == 'ce'
    assert CPU.shapes_of(a) == CPU.shapes_of(b)
    assert Model(CPU.make_args(loss='ce', compute_dtype='bf16'), 60, False).ce_dtype == 'fp32'


def test_ce_dtype_without_loss_ce_raises():
    from adapter4rec_amd.cv import Model
    with pytest.raises(NotImplementedError, match='--ce_dtype'):
        Model(CPU.make_args(loss='bce', ce_dtype='bf16'), 60, False)
    with pytest.raises(NotImplementedError, match='--ce_dtype'):
        Model(CPU.make_args(ce_dtype='bf16'), 60, False)
    Model(CPU.make_args(loss='bce', ce_dtype='fp32'), 60, False)


@pytest.fixture
def simulated_engine(monkeypatch):
    import adapter4rec_amd.engine as E
    monkeypatch.setattr(E.TransRecEngine, '_require_device', lambda self, p0: None)


def test_ce_dtype_without_loss_ce_engine_raises(simulated_engine):
    from adapter4rec_amd.cv import Model
    from adapter4rec_amd.engine_id import IdRecEngine
    with pytest.raises(NotImplementedError, match='--ce_dtype'):
        IdRecEngine(Model(CPU.make_args(), 60, False), CPU.make_args(loss='bce', ce_dtype='bf16'), arch='sasrec', dtype='fp32')


def test_ce_dtype_with_an_unserved_width_raises(simulated_engine):
    from adapter4rec_amd.cv import Model
    model = Model(CPU.make_args(loss='ce', ce_dtype='bf16', embedding_dim=32), 60, False)
    with pytest.raises(NotImplementedError, match='--ce_dtype'):
        model._engine()


def test_served_widths_and_row_group():
    from adapter4rec_amd import _lib as L
    assert L.SCORE_CE_BF16_ROWS == B16.G == 64
    assert set(L.SCORE_CE_BF16_E) <= set(L.SCORE_CE_E) and {64, 128} <= set(L.SCORE_CE_BF16_E)
    assert {E for _, _, E, _ in B16.SHAPES} == set(L.SCORE_CE_BF16_E)


@pytest.mark.parametrize('E', [64, 128])
@pytest.mark.parametrize('ranges', [1, 7, 32])
def test_workspace_does_not_grow_with_the_table(E, ranges):
    from adapter4rec_amd import _lib as L
    R = 1280
    small, large = L.score_ce_bf16_ws_bytes(R, 1000, E, ranges), L.score_ce_bf16_ws_bytes(R, 1000000, E, ranges)
    assert small == large > 0
    assert large <= ranges * R * E * 4
    assert L.score_ce_bf16_ws_bytes(R, 1000000, E, 0) <= 32 * R * E * 4 < R * 1000000 * 4


def test_workspace_is_zero_for_refused_arguments():
    from adapter4rec_amd import _lib as L
    for R, N1, E, ranges in ((0, 100, 64, 1), (16, 1, 64, 1), (16, 100, 96, 1), (16, 100, 32, 1), (16, 100, 64, 33), (16, 100, 64, -1)):
        assert L.score_ce_bf16_ws_bytes(R, N1, E, ranges) == 0
    for E in (256, 512):                                 # widths of the fp32 head the bf16 kernels do not serve
        assert (L.score_ce_bf16_ws_bytes(16, 100, E, 1) > 0) == (E in L.SCORE_CE_BF16_E)


@pytest.mark.parametrize('R,N1', [(1, 2), (64, 17), (65, 18), (1280, 14721), (1280, 500001), (100000, 40), (5, 1000001)])
def test_range_count_is_bounded(R, N1):
    from adapter4rec_amd import _lib as L
    k = L.score_ce_bf16_ranges(R, N1)
    assert 1 <= k <= 32 and k <= (N1 - 1 + 15) // 16
    with pytest.raises(ValueError):
        L.score_ce_bf16_ranges(0, N1)


# ------------------------------------------------------------------ the C boundary of the new exports (include/a4r_score_ce_bf16.h), held as
# tests/test_abi_cpu.py holds include/a4r.h: with that file's own parser and rules
def bf16_prototypes():
    import re
    import test_abi_cpu as ABI
    out = {}
    for ret, name, args in re.findall(r'\b(int|size_t)\s+(a4r_\w+)\s*\(([^;{]*?)\)\s*;', ABI.header(('include', 'a4r_score_ce_bf16.h'))):
        params = []
        for a in args.split(','):
            words = re.sub(r'\bconst\b', ' ', a).replace('*', ' * ').split()
            params.append((words[0], '*' in words))
        assert name not in out, name
        out[name] = (ret, params)
    return out


def test_signature_table_matches_the_header_and_the_library():
    import ctypes
    import re
    import test_abi_cpu as ABI
    from adapter4rec_amd import _lib as L
    protos = bf16_prototypes()
    table = L.SCORE_CE_BF16_SIGNATURES
    assert sorted(table) == sorted(protos) == ['a4r_score_ce_bf16_bwd_items', 'a4r_score_ce_bf16_bwd_rows', 'a4r_score_ce_bf16_cast', 'a4r_score_ce_bf16_fwd',
                                               'a4r_score_ce_bf16_ranges', 'a4r_score_ce_bf16_ws_bytes']
    assert not set(table) & set(L.SIGNATURES)
    for name, (ret, params) in protos.items():
        restype, argtypes = table[name]
        assert restype is ABI.SCALARS[ret] and len(argtypes) == len(params), name
        for i, (got, (ctype, ptr)) in enumerate(zip(argtypes, params)):
            assert got is ABI.expected_argtype(L, ctype, ptr), (name, i, ctype, ptr, got)
    # the argument lists are the fp32 entry points' (the two operands const void* in place of const float*)
    for name in ('ws_bytes', 'ranges', 'fwd', 'bwd_rows', 'bwd_items'):
        assert table['a4r_score_ce_bf16_' + name] == L.SIGNATURES['a4r_score_ce_' + name], name
    txt = ABI.header(('include', 'a4r_score_ce_bf16.h'))
    assert 'typedef' not in txt and int(re.search(r'#define\s+A4R_SCORE_CE_BF16_ROWS\s+(\d+)', txt).group(1)) == L.SCORE_CE_BF16_ROWS
    assert '#include "a4r_score_ce_bf16.h"' in open(ABI.os.path.join(ABI.ROOT, 'include', 'a4r.h')).read()          # one public header reaches all
    lib = ctypes.CDLL(L.LIB_PATH)
    assert all(hasattr(lib, name) for name in table)
    loaded = L.lib()                                      # lib() installs the table when it loads the library, beside SIGNATURES
    assert all(getattr(loaded, n).argtypes == a and getattr(loaded, n).restype is r for n, (r, a) in table.items())
    with pytest.raises((TypeError, ctypes.ArgumentError)):
        loaded.a4r_score_ce_bf16_ranges(16.0, 40)


def test_entry_points_refuse_null_pointers_before_launching():
    """NULL for every pointer and 0 for every scalar: A4R_EINVAL from each launch, in front of the first HIP call (so this runs without a GPU)."""
    import ctypes
    from adapter4rec_amd import _lib as L
    if torch.cuda.is_available():
        pytest.skip('argument-check probe is a CPU test')
    lib = ctypes.CDLL(L.LIB_PATH)
    probed = 0
    for name, (restype, argtypes) in L.SCORE_CE_BF16_SIGNATURES.items():
        if ctypes.c_void_p not in argtypes:
            continue
        f = getattr(lib, name)
        f.argtypes, f.restype = argtypes, restype
        assert f(*[None if t is ctypes.c_void_p else 0.0 if t is ctypes.c_float else 0 for t in argtypes]) == -1, name
        probed += 1
    assert probed == 4


def test_wrappers_marshal_what_the_header_declares(monkeypatch):
    """Every new wrapper executes its own call line against test_binding_calls_cpu's recorder, held to this module's table."""
    import test_binding_calls_cpu as BC
    from adapter4rec_amd import _lib as L
    from adapter4rec_amd import _lib_ce_bf16 as B
    rec = BC.Recorder()
    returns = dict(a4r_score_ce_bf16_ws_bytes=64, a4r_score_ce_bf16_ranges=1)

    class Stand:
        def __getattr__(self, name):
            restype, argtypes = B.SCORE_CE_BF16_SIGNATURES[name]

            def call(*args):
                assert len(args) == len(argtypes), name
                for i, (t, a) in enumerate(zip(argtypes, args)):
                    t.from_param(a)
                    if t is L._P:
                        assert a is None or a == 0 or a in rec.known, (name, i)          # (0: the stream)
                    else:
                        assert not isinstance(a, torch.Tensor) and a not in rec.known, (name, i)
                rec.calls[name] = rec.calls.get(name, 0) + 1
                return returns.get(name, 0)
            return call

    monkeypatch.setattr(L, '_lib', Stand())
    monkeypatch.setattr(L, 'require_gpu', lambda *tensors: None)
    monkeypatch.setattr(L, '_stream', lambda: 0)
    t, BF, U8, I32 = rec.tensor, torch.bfloat16, torch.uint8, torch.int32
    R, N1, E = 4, 9, 64
    prec, tbl, prec_b, tbl_b = t(R, E), t(N1, E), t(R, E, dtype=BF), t(N1, E, dtype=BF)
    tgt, mask, lse, lw = t(R, dtype=I32), t(R), t(R), t(4)
    L.cast_bf16(tbl, tbl_b)
    L.cast_bf16(prec, prec_b, np.int64(R * E))
    assert L.score_ce_bf16_ranges(R, N1) == 1 and L.score_ce_bf16_ws_bytes(R, N1, E) == 64 and L.score_ce_bf16_ws_bytes(R, N1, E, ranges=2) == 64
    L.score_ce_bf16_fwd(prec_b, tbl_b, tgt, mask, lse, t(R), lw, R, ws=t(64, dtype=U8))
    L.score_ce_bf16_fwd(prec_b, tbl_b, tgt, mask, lse, t(R), lw, np.int64(R), ranges=2, ws=t(64, dtype=U8))
    L.score_ce_bf16_bwd(prec_b, tbl_b, tgt, mask, lse, lw, 1.0, t(R, E), None, R, ws=t(64, dtype=U8))                # the rows launch alone
    assert rec.calls['a4r_score_ce_bf16_bwd_rows'] == 1 and 'a4r_score_ce_bf16_bwd_items' not in rec.calls
    L.score_ce_bf16_bwd(prec_b, tbl_b, tgt, mask, lse, lw, 1.0, None, t(N1, E), R)                                    # the items launch alone
    L.score_ce_bf16_bwd(prec_b, tbl_b, tgt, mask, lse, lw, 1.0, t(R, E), t(N1, E), R, ranges=2, scale_dev=t(1), ws=t(64, dtype=U8))
    assert rec.calls['a4r_score_ce_bf16_bwd_rows'] == 2 and rec.calls['a4r_score_ce_bf16_bwd_items'] == 2
    assert sorted(rec.calls) == sorted(B.SCORE_CE_BF16_SIGNATURES)
    with pytest.raises(AssertionError):                  # fp32 operands are refused by the wrapper itself
        L.score_ce_bf16_fwd(prec, tbl, tgt, mask, lse, t(R), lw, R, ws=t(64, dtype=U8))


def test_either_binding_module_can_be_imported_first():
    """_lib_ce_bf16 uses _lib and _lib hands out _lib_ce_bf16's names: a fresh interpreter (this test is about import order) imports the new module
    first, then reaches the same objects through _lib, whose own table and namespace stay what they were."""
    import subprocess
    import sys
    import test_abi_cpu as ABI
    code = ('import adapter4rec_amd._lib_ce_bf16 as B; from adapter4rec_amd import _lib as L; '
            'assert L.cast_bf16 is B.cast_bf16 and L.SCORE_CE_BF16_E == (64, 128) and L.score_ce_bf16_ws_bytes(16, 100, 64, 1) == 4096; '
            'assert "cast_bf16" not in vars(L) and not set(B.SCORE_CE_BF16_SIGNATURES) & set(L.SIGNATURES); '
            'assert L.lib().a4r_score_ce_bf16_cast.argtypes == B.SCORE_CE_BF16_SIGNATURES["a4r_score_ce_bf16_cast"][1]')
    subprocess.check_call([sys.executable, '-c', code], cwd=ABI.ROOT)
    from adapter4rec_amd import _lib as L
    with pytest.raises(AttributeError):
        L.score_ce_bf16_nothing
