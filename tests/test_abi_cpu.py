"""CPU: the C boundary.  include/a4r.h is the single source: liba4r_hip.so exports every symbol it declares, and the binding's signature table,
struct mirrors and constants (adapter4rec_amd/_lib.py) agree with it prototype by prototype and field by field (no compute calls)."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCALARS = {'int': ctypes.c_int, 'int32_t': ctypes.c_int, 'int64_t': ctypes.c_int64, 'uint32_t': ctypes.c_uint32, 'uint64_t': ctypes.c_uint64,
           'float': ctypes.c_float, 'long': ctypes.c_long, 'size_t': ctypes.c_size_t}
MIRRORS = dict(a4r_gemm_t='GemmArgs', a4r_attn_t='AttnArgs', a4r_pack_desc_t='PackDesc', a4r_phm_desc_t='PhmDesc', a4r_layer_adapter_t='LayerAdapter',
               a4r_encoder_layer_t='EncoderLayer', a4r_sasrec_block_t='SasrecBlock', a4r_add_desc_t='AddDesc', a4r_tn_prob_t='TnProb',
               a4r_lora_desc_t='LoraDesc')
DEVICE_TABLES = ('a4r_pack_desc_t', 'a4r_phm_desc_t', 'a4r_add_desc_t', 'a4r_lora_desc_t')    # descriptor arrays in DEVICE memory: passed as an address
MIXED = ('a4r_gemm_t', 'a4r_encoder_layer_t', 'a4r_sasrec_block_t')                           # 4- and 8-byte members interleaved: every offset is probed


def header(path=('include', 'a4r.h')):
    txt = open(os.path.join(ROOT, *path)).read()
    return re.sub(r'//[^\n]*', '', re.sub(r'/\*.*?\*/', '', txt, flags=re.S))


def prototypes():
    """name -> (return type, [(type, is_pointer)] per parameter) for every prototype of the header."""
    out = {}
    for ret, name, args in re.findall(r'\b(int|size_t)\s+(a4r_\w+)\s*\(([^;{]*?)\)\s*;', header()):
        params = []
        for a in ([] if args.strip() in ('', 'void') else args.split(',')):
            words = re.sub(r'\bconst\b', ' ', a).replace('*', ' * ').split()
            params.append((words[0], '*' in words))
        assert name not in out, name
        out[name] = (ret, params)
    return out


def structs():
    """struct name -> [(field, type, is_pointer, array length or 0)] for every `typedef struct { ... } a4r_*_t;` of the header."""
    out = {}
    for body, name in re.findall(r'typedef\s+struct\s*\w*\s*\{(.*?)\}\s*(a4r_\w+_t)\s*;', header(), flags=re.S):
        fields = []
        for decl in filter(None, (d.strip() for d in body.split(';'))):
            base, rest = re.match(r'(?:const\s+)?(\w+)\s*(.*)$', decl, flags=re.S).groups()
            for d in rest.split(','):
                m = re.match(r'\s*(\*?)\s*(\w+)\s*(?:\[(\d+)\])?\s*$', d)
                fields.append((m.group(2), base, bool(m.group(1)), int(m.group(3) or 0)))
        out[name] = fields
    return out


def declared():
    return sorted(prototypes())


def expected_argtype(L, ctype, ptr):
    if not ptr:
        return SCALARS[ctype]
    if ctype in MIRRORS and ctype not in DEVICE_TABLES:
        return ctypes.POINTER(getattr(L, MIRRORS[ctype]))
    return ctypes.c_void_p


def check_table(L, table):
    protos = prototypes()
    assert sorted(table) == sorted(protos)
    for name, (ret, params) in protos.items():
        restype, argtypes = table[name]
        assert restype is SCALARS[ret], name
        assert len(argtypes) == len(params), name
        for i, (got, (ctype, ptr)) in enumerate(zip(argtypes, params)):
            assert got is expected_argtype(L, ctype, ptr), (name, i, ctype, ptr, got)


def check_mirror(L, cname, fields):
    want = []
    for fname, ctype, ptr, n in structs()[cname]:
        t = ctypes.c_void_p if ptr else getattr(L, MIRRORS[ctype]) if ctype in MIRRORS else SCALARS[ctype]
        want.append((fname, t * n if n else t))
    assert [(f[0], f[1]) for f in fields] == want, cname


def test_header_declares_entry_points():
    names = declared()
    assert 'a4r_gemm_nt' in names and 'a4r_attn_bwd' in names and len(names) >= 19
    assert set(structs()) == set(MIRRORS)


def test_library_exports_every_declared_symbol():
    from adapter4rec_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.fail(f'{_lib.LIB_PATH} missing: run __graft_entry__.build()')
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in declared():
        assert hasattr(lib, name), name
    assert sorted(_lib.EXPORTS) == declared() == sorted(_lib.SIGNATURES)
    want = int(re.search(r'#define A4R_ABI_VERSION (\d+)', header()).group(1))
    assert lib.a4r_version() == want == _lib.ABI_VERSION


def test_signature_table_matches_every_prototype():
    """Every export's restype and every position's argtype is the kind the header declares: pointers c_void_p (POINTER(mirror) for the structs the
    host fills), int / int32_t c_int, int64_t c_int64, uint32_t, uint64_t, float, long, size_t exactly those."""
    from adapter4rec_amd import _lib as L
    check_table(L, L.SIGNATURES)
    # the check has teeth: two neighbouring parameters of different kind swapped in one signature (a copy; the module is not touched)
    res, args = L.SIGNATURES['a4r_rows_idx_copy']
    assert args[4] is not args[5]
    with pytest.raises(AssertionError):
        check_table(L, dict(L.SIGNATURES, a4r_rows_idx_copy=(res, args[:4] + (args[5], args[4]) + args[6:])))
    with pytest.raises(AssertionError):                                                      # a dropped parameter, a missing entry
        check_table(L, dict(L.SIGNATURES, a4r_rows_idx_copy=(res, args[:-1])))
    with pytest.raises(AssertionError):
        check_table(L, {k: v for k, v in L.SIGNATURES.items() if k != 'a4r_id_sample'})


def test_struct_mirrors_match_the_header_field_by_field():
    """All ten mirrors: the same field names in the same order with the same kinds (pointer members c_void_p, `ad[2]` an array of its mirror)."""
    from adapter4rec_amd import _lib as L
    for cname, pyname in MIRRORS.items():
        check_mirror(L, cname, getattr(L, pyname)._fields_)
    # teeth: two same-sized neighbouring fields swapped (sizeof and every other offset unchanged), on a copy
    f = list(L.AddDesc._fields_)
    i = [n for n, _ in f].index('rows')
    assert f[i][1] is f[i + 1][1]
    f[i], f[i + 1] = f[i + 1], f[i]
    with pytest.raises(AssertionError):
        check_mirror(L, 'a4r_add_desc_t', f)


def test_binding_struct_sizes_match_header():
    """ctypes mirrors of the ABI structs must have the C layout (checked against a gcc-compiled probe): sizeof of all ten, offsetof of every field of
    the three that mix 4- and 8-byte members."""
    from adapter4rec_amd import _lib
    S = structs()
    exprs = [f'sizeof({c})' for c in MIRRORS] + [f'offsetof({c}, {f[0]})' for c in MIXED for f in S[c]]
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "a4r.h"\nint main(){' + ''.join(f'printf("%zu\\n", {e});' for e in exprs) + 'return 0;}\n'
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, 'p.c'), 'w').write(src)
        subprocess.check_call(['gcc', '-I', os.path.join(ROOT, 'include'), os.path.join(d, 'p.c'), '-o', os.path.join(d, 'p')])
        out = subprocess.check_output([os.path.join(d, 'p')]).decode().split()
    want = [ctypes.sizeof(getattr(_lib, MIRRORS[c])) for c in MIRRORS] + [getattr(getattr(_lib, MIRRORS[c]), f[0]).offset for c in MIXED for f in S[c]]
    assert len(want) == 10 + sum(len(S[c]) for c in MIXED) > 10 + 3 * 30 and [int(x) for x in out] == want


def test_mirrored_constants_equal_their_defines():
    from adapter4rec_amd import _lib as L
    d = {k: int(v) for k, v in re.findall(r'#define\s+A4R_(\w+)\s+\(?(-?\d+)\)?\s', header())}
    names = ('BF16', 'F32', 'FP8', 'ACT_NONE', 'ACT_RELU', 'ACT_GELU', 'ACT_GELU_TANH', 'ACT_LEAKY', 'DACT_MUL', 'DACT_MUL_Q8', 'ABI_VERSION',
             'EVAL_MAX_HISTORY', 'ID_SUM_CHUNK', 'TOPK_MAX_K', 'GRAD_NORM_PARTS', 'SCORE_CE_MAX_RANGES')
    assert {n: getattr(L, n) for n in names} == {n: d[n] for n in names}
    assert set(L.ACT_BY_NAME.values()) <= {d[n] for n in d if n.startswith('ACT_')}
    # the two constants of a4r_id_sample that the header states in prose: their definitions in the C sources
    common = header(('adapter4rec_amd', 'csrc', 'a4r_common.h'))
    assert L.SAMPLE_SITE == int(re.search(r'#define\s+A4R_SAMPLE_SITE\s+(\d+)u?\b', common).group(1))
    sample = header(('adapter4rec_amd', 'csrc', 'a4r_sample.hip'))
    assert L.SAMPLE_MAX_L == int(re.search(r'constexpr\s+int\s+SAMPLE_MAX_L\s*=\s*(\d+)\s*;', sample).group(1))


def test_every_entry_point_refuses_null_pointers_before_launching():
    """Error behaviour at the boundary: called with NULL for every pointer and 0 for every scalar (the two argument structs zero-filled), each
    entry point that takes a pointer returns A4R_EINVAL (include/a4r.h) -- the checks sit in front of the first HIP call, so this runs without a GPU
    and nothing is enqueued.  (a4r_gemm_tail_plan is a host-side query whose outputs are optional: it returns its flag.)  The argument types are
    the binding's own table."""
    import torch
    from adapter4rec_amd import _lib
    if torch.cuda.is_available():
        pytest.skip('argument-check probe is a CPU test')
    codes = dict(re.findall(r'#define (A4R_OK|A4R_EINVAL|A4R_ELAUNCH) \(?(-?\d+)\)?', header()))
    assert {k: int(v) for k, v in codes.items()} == dict(A4R_OK=0, A4R_EINVAL=-1, A4R_ELAUNCH=-2)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    zero_filled = [ctypes.POINTER(t) for t in (_lib.GemmArgs, _lib.AttnArgs, _lib.EncoderLayer)]
    probed = 0
    for name, (restype, argtypes) in _lib.SIGNATURES.items():
        pointers = [t for t in argtypes if t is ctypes.c_void_p or hasattr(t, 'contents')]
        if not pointers or name == 'a4r_gemm_tail_plan':
            continue
        vals = []
        for t in argtypes:
            if t in zero_filled:
                vals.append(ctypes.pointer(t._type_()))
            elif t in pointers:
                vals.append(None)
            else:
                vals.append(0.0 if t is ctypes.c_float else 0)
        f = getattr(lib, name)
        f.argtypes, f.restype = argtypes, restype
        assert f(*vals) == -1, name
        probed += 1
    assert probed >= 44, probed


def test_no_cpu_fallback():
    import torch
    from adapter4rec_amd import _lib
    a = torch.zeros(128, 64)
    with pytest.raises(RuntimeError):
        _lib.gemm_nt(a, a, a)


def test_pack_fragment_layouts_are_permutations_of_the_kernels_read_order():
    """a4r_pack_desc_t layouts 1 / 2 (ABI 408), restated in tests/sim_lib.py: frag_index must be a permutation of the destination, and element
    (wave w, step s, [row tile nt | half h, step ks], lane, j) must be the matrix element the one-launch adapter kernels load for that fragment
    from a ROW-major copy (csrc/a4r_adapter_fused.hip: the two address forms of wd / wu)."""
    import torch
    import sim_lib
    for H in (128, 256, 512, 768, 1024):
        NW = 4 if H == 128 else 8
        CW, KS = H // NW, H // NW // 32
        i1, i2 = sim_lib.frag_index(1, 64, H), sim_lib.frag_index(2, H, 64)
        assert sorted(i1.reshape(-1).tolist()) == list(range(64 * H)) and sorted(i2.reshape(-1).tolist()) == list(range(64 * H))
        for w in (0, NW - 1):
            for lane in (0, 17, 63):
                fr, kg = lane & 15, lane >> 4
                for s in range(KS):
                    for nt in range(4):        # forward wd[s][nt] / backward wu[s][nt]: row nt*16 + fr, columns w*CW + s*32 + kg*8 + j
                        for j in (0, 7):
                            assert int(i1[nt * 16 + fr, w * CW + s * 32 + kg * 8 + j]) == ((((w * KS + s) * 4 + nt) * 64 + lane) * 8 + j)
                    for h in range(2):
                        for ks in range(2):    # forward wu[2s+h][ks] / backward image: row w*CW + s*32 + (fr>>2)*8 + h*4 + (fr&3), columns ks*32 + kg*8 + j
                            for j in (0, 7):
                                r = w * CW + s * 32 + (fr >> 2) * 8 + h * 4 + (fr & 3)
                                assert int(i2[r, ks * 32 + kg * 8 + j]) == (((((w * KS + s) * 2 + h) * 2 + ks) * 64 + lane) * 8 + j)

