"""csrc/shade_common.h holds the shading arithmetic of the compositing, relighting and traced-surface kernels once (DESIGN
section 4.23): every helper it defines has no second definition under csrc/, and the clamped quotients it owns are written
nowhere else.  Reads the sources only."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "object-intrinsics_amd", "csrc")
DEFINITION = re.compile(r"^__device__ __forceinline__ [\w:]+ (\w+)\(", re.M)
# a loader over the shared helper of the same name: unit_normal(grad, k, ...) reads gradient row k
LOADERS = {"unit_normal": ["trace_common.h"]}
# shade_common.h's own overloads: the unit normal from three components, and from three components and |g|
OVERLOADS = {"unit_normal": 2}


def _sources():
    return {f: open(os.path.join(CSRC, f)).read() for f in sorted(os.listdir(CSRC)) if f.endswith((".h", ".hip"))}


def test_shade_helpers_are_defined_once():
    src = _sources()
    names = DEFINITION.findall(src["shade_common.h"])
    assert sorted(set(names)) == ["anneal_cos", "inv_s_of", "light_dir", "light_terms", "neus_alpha", "normalize3", "phong_geometry",
                                  "transmittance_step", "unit_normal", "unit_view"]
    for name in set(names):
        holders = sorted(f for f, text in src.items() for n in DEFINITION.findall(text) if n == name)
        assert holders == sorted(["shade_common.h"] * OVERLOADS.get(name, 1) + LOADERS.get(name, [])), (name, holders)
    # each of them is called outside the header
    for name in set(names):
        assert any(re.search(r"\b" + name + r"\(", text) for f, text in src.items() if f != "shade_common.h"), name


def test_clamped_quotients_stand_in_shade_common_alone():
    src = _sources()
    at = lambda pattern: sorted((f, line.strip()) for f, text in src.items() for line in text.splitlines() if re.search(pattern, line))
    # the unit normal n = g / max(|g|, 1e-6).  render_bwd.hip differentiates the norm itself: it takes |g| as sqrtf alone and
    # branches on |g| > 1e-6, so no line of it restates the clamped quotient's divisor.
    assert at(r"fmaxf\(sqrtf\(.*1e-6f") == [
        ("shade_common.h", "const float gnc = fmaxf(sqrtf(gx * gx + gy * gy + gz * gz), 1e-6f);"),
    ]
    # every other clamp at 1e-6: the normal's divisor from |g|, the view vector's and the light's eps, inv_s; mesh_attr.hip's
    # normal multiplies by the reciprocal (another rounding) and stays its own
    assert at(r"fmaxf\([^;]*1e-6f|normalize3\([^;]*1e-6f\)") == [
        ("envlight.hip", "normalize3(x, y, z, 1e-6f);"),
        ("mesh_attr.hip", "const float inv = 1.0f / fmaxf(gn, 1e-6f);"),
        ("render.hip", "normalize3(lx, ly, lz, 1e-6f);"),
        ("render_bwd.hip", "normalize3(lx, ly, lz, 1e-6f);"),
        ("render_bwd.hip", "normalize3(v[0], v[1], v[2], 1e-6f);"),
        ("scene_light.hip", "normalize3(x, y, z, 1e-6f);"),
        ("shade_common.h", "const float gnc = fmaxf(gn, 1e-6f);"),
        ("shade_common.h", "const float gnc = fmaxf(sqrtf(gx * gx + gy * gy + gz * gz), 1e-6f);"),
        ("shade_common.h", "normalize3(lx, ly, lz, 1e-6f);"),
        ("shade_common.h", "normalize3(vx, vy, vz, 1e-6f);"),
        ("shade_common.h", "s.v = fminf(fmaxf(s.raw, 1e-6f), 1e6f);"),
    ]
    # no comment explains code as another kernel's expressions: the call says it
    assert at(r"(composite_fwd_kernel|relight_kernel|gen_rays_kernel)'s (expression|normalisation)|(render|relight)\.hip's (helper|normal)|"
              r"surface_shade_at's normal") == []
