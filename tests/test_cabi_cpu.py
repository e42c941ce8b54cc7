"""CPU-only checks of the drop-in boundary: the C-ABI library builds/loads, exports every symbol that
include/oi_hip.h declares and binds each as declared (tests/helpers/cabi.py, with that helper's own negative checks), and
the host modules import and keep the reference's names (no compute)."""
import ctypes
import types

import pytest
import torch

from helpers import cabi


def test_library_exports_every_declared_symbol():
    lib, L = cabi.built_lib()
    names, mirrors = cabi.check_header("oi_hip.h", lib)
    assert len(names) >= 25
    assert mirrors == ["PrepParams", "CompositeParams", "CompositeGrads"]
    assert L.oi_arch() == b"gfx950"
    assert L.oi_mlp_packed_bytes(0) == 2816 * 4 + 16 * 65536 + 8 * 65536  # header, 16 MFMA images, 8 plain fp32 matrices
    assert L.oi_mlp_packed_bytes(2) == 2816 * 4 + 16 * 32768 + 8 * 65536
    assert L.oi_mlp_packed_bytes(3) == 2816 * 4 + 16 * 98304 + 8 * 65536


def test_every_mirror_is_checked_against_its_header():
    lib, _ = cabi.built_lib()
    checked = [m for h in lib.SIGS for m in cabi.check_header(h, lib)[1]]
    assert sorted(checked) == sorted(n for n, c in vars(lib).items() if isinstance(c, type) and issubclass(c, ctypes.Structure))
    assert sorted(checked) == ["CompositeGrads", "CompositeParams", "EnvShadeBounceParams", "EnvShadeParams", "PrepParams",
                               "RelightParams", "SceneOcclusionParams", "SceneShadeAoParams", "SceneShadeParams", "SurfaceAoParams",
                               "SurfaceParams", "TraceBatch", "TraceState"]


def test_no_struct_mirror_outside_lib():
    """Every ctypes.Structure of the package stands in oi_amd.lib, where the test above finds it, and under no second name
    elsewhere: a mirror in another module would be bound as a plain pointer and held against no header."""
    import importlib
    import os
    cabi.built_lib()
    import oi_amd
    names = sorted("oi_amd." + f[:-3] for f in os.listdir(os.path.dirname(oi_amd.__file__)) if f.endswith(".py") and f != "__init__.py")
    assert "oi_amd.lib" in names and "oi_amd.ops" in names and len(names) >= 10
    for name in names:
        mod = importlib.import_module(name)
        found = sorted(n for n, c in vars(mod).items() if isinstance(c, type) and issubclass(c, ctypes.Structure))
        assert found == [] or name == "oi_amd.lib", f"{name} holds the struct mirrors {found}: they belong in oi_amd.lib alone"


HEADER_FIXTURE = """
#define OI_ROWS 8
typedef void* oi_stream_t; /* a stream */
typedef struct oi_pair_params {
  float m[OI_ROWS][16], v[3];  // arrays
  long long N;
  int A, B;
  const float *src, *dst;
} oi_pair_params;
typedef struct oi_not_mirrored { int x; } oi_not_mirrored;
int oi_pair(const oi_pair_params* p, const float* x, long long n, unsigned seed, oi_stream_t stream);
size_t oi_pair_bytes(int n, double scale);  /* int oi_in_a_comment(int n); */
const char* oi_pair_name(void);
void oi_pair_free(oi_not_mirrored** p);
"""


_vp, _i, _ll, _f, _u = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong, ctypes.c_float, ctypes.c_uint
PAIR_FIELDS = dict(m=(_f * 16) * 8, v=_f * 3, N=_ll, A=_i, B=_i, src=_vp, dst=_vp)


def _mirror(**changes):
    return type("PairParams", (ctypes.Structure,), {"_fields_": list({**PAIR_FIELDS, **changes}.items())})


PAIR = _mirror()


def _fixture_lib(mirror=PAIR, other="oi_other", **changes):
    """A stand-in for oi_amd.lib that binds HEADER_FIXTURE correctly, but for `changes`."""
    sigs = {"oi_pair": (_i, [ctypes.POINTER(mirror), _vp, _ll, _u, _vp]), "oi_pair_bytes": (ctypes.c_size_t, [_i, ctypes.c_double]),
            "oi_pair_name": (ctypes.c_char_p, []), "oi_pair_free": (None, [_vp]), **changes}
    table = {"fixture.h": sigs, "other.h": {other: (_i, [])}}
    return types.SimpleNamespace(SIGS=table, symbols=lambda h: sorted(table[h]), PairParams=mirror,
                                 load=lambda: types.SimpleNamespace(**{n: None for n in sigs}))


def test_contract_helper_refuses_what_it_must():
    check = lambda text=HEADER_FIXTURE, **changes: cabi.check_header("fixture.h", _fixture_lib(**changes), text)
    assert check() == (["oi_pair", "oi_pair_bytes", "oi_pair_name", "oi_pair_free"], ["PairParams"])
    pair = lambda *args: {"oi_pair": (_i, list(args))}
    P = ctypes.POINTER(PAIR)
    edit = lambda old, new: dict(text=HEADER_FIXTURE.replace(old, new))
    bad = [
        (edit("unsigned seed,", "unsigned seed, int extra,"), "oi_pair: 6 parameters, 5 bound"),    # one argument more
        (pair(P, _vp, _i, _u, _vp), "oi_pair: parameter 2"),                                        # long long bound as c_int
        (pair(_vp, _vp, _ll, _u, _vp), "oi_pair: parameter 0"),                                     # a mirrored struct as void*
        (pair(ctypes.POINTER(_mirror()), _vp, _ll, _u, _vp), "oi_pair: parameter 0"),               # another struct's pointer
        (pair(P, _vp, _ll, _i, _vp), "oi_pair: parameter 3"),                                       # unsigned bound as c_int
        (pair(P, _ll, _ll, _u, _vp), "oi_pair: parameter 1"),                                       # a pointer bound as an integer
        ({"oi_pair_bytes": (_i, [_i, ctypes.c_double])}, "oi_pair_bytes: returns"),
        ({"oi_pair_bytes": (ctypes.c_size_t, [_i, _f])}, "oi_pair_bytes: parameter 1"),             # double bound as c_float
        ({"oi_pair_free": (_i, [_vp])}, "oi_pair_free: returns"),
        (dict(other="oi_pair_name"), "oi_pair_name stands under fixture.h and other.h"),
        (edit("const char* oi_pair_name(void);", ""), "oi_pair_name"),                              # bound, not declared
        (edit("void oi_pair_free", "int oi_new(int n);\nvoid oi_pair_free"), "oi_new"),              # declared, not bound
        (edit("int n, double scale", "int n, long scale"), "unknown type 'long'"),
        (edit("int A, B;", "int B, A;"), "oi_pair_params: fields"),                                 # two fields swapped
        (dict(mirror=_mirror(N=_i)), "oi_pair_params.N"),
        (dict(mirror=_mirror(m=(_f * 8) * 16)), "oi_pair_params.m"),                                # the extents the other way round
        (dict(mirror=_mirror(v=_i * 3)), "oi_pair_params.v"),
        (dict(mirror=_mirror(dst=_ll)), "oi_pair_params.dst"),
    ]
    for kw, message in bad:
        with pytest.raises(AssertionError, match=message):
            check(**kw)


def test_ops_fail_loudly_without_gpu_tensors():
    from oi_amd import ops, lib
    with pytest.raises(lib.OiHipError):
        ops.midpoints(torch.zeros(4, 3), torch.zeros(4, 3), torch.zeros(4, 8), 0.1)


def test_modules_mirror_reference_names():
    from oi_amd.config import TARGET_MAP, get_obj_from_str
    for ref_target in TARGET_MAP:
        assert get_obj_from_str(ref_target) is not None
    from oi_amd.fields import ShapeNetwork, ColorNetwork, SingleVarianceNetwork
    from oi_amd.discriminator import ADADiscriminatorView
    s = ShapeNetwork(None, D=8, W=128, input_ch=3, input_ch_views=3, style_dim=64)
    assert sum(p.numel() for p in s.parameters()) + sum(
        p.numel() for p in ColorNetwork(D=8, W=128, input_ch=3, input_ch_views=3, style_dim=64).parameters()) + 1 + 6 == 295755
    for m in ("style", "forward", "sdf", "gradient", "pts_linears", "sigma_linear"):
        assert hasattr(s, m)
    d = ADADiscriminatorView(out_dim_position=6, out_dim_latent=0,
                             aug={"__target__": "src.third_party.ada.augment.AugmentPipe", "kwargs": {"scale": 1, "xint": 1}},
                             aug_p=1, img_size=128, in_dim=3, last_bias=False, n_feat=512, out_dim=7)
    assert sum(p.numel() for p in d.parameters()) == 2844160
    import copy
    copy.deepcopy(s)  # EMA copies (src/utils/ema.py:11-12)


def test_unsupported_configurations_raise():
    from oi_amd.fields import ShapeNetwork
    from oi_amd.augment import AugmentPipe
    with pytest.raises(NotImplementedError):
        ShapeNetwork(None, D=8, W=256, input_ch=3, input_ch_views=3, style_dim=64)
    with pytest.raises(NotImplementedError):
        AugmentPipe(brightness=1)
