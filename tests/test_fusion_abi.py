"""CPU: the C ABI of TSDF fusion and the isosurface (include/gs_fusion.h) and its binding (fusion.py)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "gs_fusion.h")
PKG = os.path.join(ROOT, "taichi_3d_gaussian_splatting_amd")
NAMES = ["gs_isosurface_emit", "gs_isosurface_plan", "gs_tsdf_integrate"]
STRUCTS = {"gs_tsdf_volume": "GsTsdfVolume", "gs_tsdf_view": "GsTsdfView", "gs_iso_volume": "GsIsoVolume"}
INVALID = -1                                                      # GS_ERR_INVALID_ARGUMENT
NAN, INF = float("nan"), float("inf")


def _prototypes():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    src = re.sub(r"typedef struct.*?\}\s*\w+;", "", src, flags=re.S)
    protos = {}
    for ret, name, params in re.findall(r"([A-Za-z_][\w ]*?[\w*])\s+(gs_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", src):
        types = [re.sub(r"\bconst\b|\s", "", re.match(r"(.*?)(\w+)$", p.strip()).group(1)) for p in params.split(",")]
        protos[name] = (ret.strip(), types)
    return protos


def _define(name):
    return int(re.search(r"#define\s+%s\s+(\d+)" % name, open(HEADER).read()).group(1))


def test_header_is_plain_c99_and_declares_the_three_functions(tmp_path):
    src = tmp_path / "probe.c"
    src.write_text(f'#include "{HEADER}"\n'
                   'int main(void) {\n'
                   '  int (*f)(gs_ctx*, const gs_tsdf_volume*, const gs_tsdf_view*, int32_t, gs_stream) = gs_tsdf_integrate;\n'
                   '  int (*g)(gs_ctx*, const gs_iso_volume*, void*, void*, int64_t*, gs_stream) = gs_isosurface_plan;\n'
                   '  int (*h)(gs_ctx*, const gs_iso_volume*, const void*, const void*, void*, int64_t, int64_t, float*, float*, int32_t*,\n'
                   '           gs_stream) = gs_isosurface_emit;\n'
                   '  (void)f; (void)g; (void)h; return GS_ISO_CELL_WS_BYTES(3) == 6 ? 0 : 1; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-c", str(src), "-o", str(tmp_path / "probe.o")])
    assert sorted(_prototypes()) == NAMES


def test_library_exports_the_symbols_and_the_main_header_is_unchanged():
    from taichi_3d_gaussian_splatting_amd import _native
    L = _native.lib()
    for n in NAMES:
        assert hasattr(L, n), f"libgsrast.so does not export {n}"
        assert n not in _native.SYMBOLS
    assert L.gs_abi_version() == _native.ABI_VERSION == 9
    assert len(L.gs_kernel_names().decode().split(",")) == 13
    main = open(os.path.join(ROOT, "include", "gs_rasterizer.h")).read().lower()
    assert "tsdf" not in main and "isosurface" not in main


def test_argtypes_match_the_prototypes():
    from taichi_3d_gaussian_splatting_amd import _native, fusion
    fusion._bind()
    L = _native.lib()
    kinds = {"gs_ctx*": C.c_void_p, "void*": C.c_void_p, "float*": C.c_void_p, "int32_t*": C.c_void_p, "int64_t*": C.c_void_p,
             "gs_stream": C.c_void_p, "int32_t": C.c_int32, "int64_t": C.c_int64,
             "gs_tsdf_volume*": C.POINTER(fusion.GsTsdfVolume), "gs_tsdf_view*": C.POINTER(fusion.GsTsdfView),
             "gs_iso_volume*": C.POINTER(fusion.GsIsoVolume)}
    protos = _prototypes()
    assert sorted(fusion.ARGTYPES) == NAMES
    for name in NAMES:
        ret, params = protos[name]
        assert ret == "int" and params[-1] == "gs_stream"          # _native.call() appends the stream
        assert name not in _native._STREAMLESS
        fn = getattr(L, name)
        assert fn.restype is C.c_int
        assert list(fn.argtypes) == [kinds[p] for p in params] == fusion.ARGTYPES[name], name


def test_struct_mirrors_match_the_compiler(tmp_path):
    """sizeof and every offsetof of the three structs, from a gcc probe of the header"""
    from taichi_3d_gaussian_splatting_amd import fusion
    lines = []
    for c_name, py_name in STRUCTS.items():
        cls = getattr(fusion, py_name)
        lines.append(f'printf("{c_name} %zu", sizeof({c_name}));')
        lines += [f'printf(" %zu", offsetof({c_name}, {field}));' for field, _ in cls._fields_]
        lines.append('printf("\\n");')
    src = tmp_path / "layout.c"
    src.write_text(f'#include <stdio.h>\n#include <stddef.h>\n#include "{HEADER}"\nint main(void) {{\n' + "\n".join(lines) + "\nreturn 0; }\n")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", str(src), "-o", str(tmp_path / "layout")])
    out = subprocess.check_output([str(tmp_path / "layout")], text=True).splitlines()
    assert len(out) == len(STRUCTS)
    for line, (c_name, py_name) in zip(out, STRUCTS.items()):
        cls = getattr(fusion, py_name)
        got = line.split()
        assert got[0] == c_name
        assert int(got[1]) == C.sizeof(cls), c_name
        assert [int(x) for x in got[2:]] == [getattr(cls, field).offset for field, _ in cls._fields_], c_name
    # the fields of the header's structs, by name and in order
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for c_name, py_name in STRUCTS.items():
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (c_name, c_name), text, flags=re.S).group(1)
        names = [n for decl in body.split(";") if decl.strip() for n in re.findall(r"(\w+)(?:\[\d+\])*\s*(?:,|$)", decl.strip())]
        assert names == [field for field, _ in getattr(fusion, py_name)._fields_], c_name


def _volume(fusion, buf, **over):
    p = C.cast(buf, C.c_void_p).value
    f = dict(tsdf=p, weight=p, colour=None, nx=4, ny=3, nz=2, origin=(C.c_float * 3)(0, 0, 0), voxel=(C.c_float * 3)(.1, .1, .1),
             trunc=0.3, max_weight=8.0, min_alpha=0.5, near=0.1)
    f.update(over)
    return fusion.GsTsdfVolume(**f)


def _view(fusion, buf, **over):
    p = C.cast(buf, C.c_void_p).value
    f = dict(depth=p, alpha=None, image=None, h=4, w=4, fx=10.0, fy=10.0, cx=2.0, cy=2.0)
    f.update(over)
    v = fusion.GsTsdfView(**f)
    for r in range(3):
        v.m[r][r] = 1.0
    return v


def _iso(fusion, buf, **over):
    p = C.cast(buf, C.c_void_p).value
    f = dict(values=p, valid=None, colour=None, nx=4, ny=3, nz=2, origin=(C.c_float * 3)(0, 0, 0), spacing=(C.c_float * 3)(.1, .1, .1),
             level=0.0, flip=0)
    f.update(over)
    return fusion.GsIsoVolume(**f)


def _three(a, b, c):
    return (C.c_float * 3)(a, b, c)


def test_integrate_refuses_bad_arguments_without_a_gpu():
    """argument checks come before anything that needs a device"""
    from taichi_3d_gaussian_splatting_amd import _native, fusion
    fusion._bind()
    f, err = _native.lib().gs_tsdf_integrate, _native.lib().gs_last_error
    buf = (C.c_float * 64)()
    views = lambda *v: (fusion.GsTsdfView * len(v))(*v)
    good = views(_view(fusion, buf))
    assert f(None, _volume(fusion, buf), good, 1, None) == INVALID and b"ctx is NULL" in err()
    ctx = C.c_void_p(8)       # a context handle that is never dereferenced: everything below is refused (or empty) before it is looked at
    assert f(ctx, None, good, 1, None) == INVALID and b"volume is NULL" in err()
    assert f(ctx, _volume(fusion, buf), good, -1, None) == INVALID and b"n_views" in err()
    assert f(ctx, _volume(fusion, buf), None, 1, None) == INVALID and b"views is NULL" in err()
    for dims in (dict(nx=-1), dict(ny=-1), dict(nz=-1)):
        assert f(ctx, _volume(fusion, buf, **dims), good, 1, None) == INVALID and b"dimension" in err()
    for dims in (dict(nx=1025, ny=1024, nz=1024), dict(nx=2 ** 31 - 1, ny=2 ** 31 - 1, nz=2 ** 31 - 1), dict(nx=2 ** 16, ny=2 ** 15, nz=1)):
        assert f(ctx, _volume(fusion, buf, **dims), good, 1, None) == INVALID and b"GS_FUSION_MAX_VOXELS" in err()
    for bad in (0.0, -0.1, NAN, INF):
        for axis in range(3):
            step = [0.1, 0.1, 0.1]
            step[axis] = bad
            assert f(ctx, _volume(fusion, buf, voxel=_three(*step)), good, 1, None) == INVALID and b"voxel" in err()
        assert f(ctx, _volume(fusion, buf, trunc=bad), good, 1, None) == INVALID and b"trunc" in err()
        assert f(ctx, _volume(fusion, buf, max_weight=bad), good, 1, None) == INVALID and b"max_weight" in err()
    assert f(ctx, _volume(fusion, buf, origin=_three(0, NAN, 0)), good, 1, None) == INVALID and b"origin" in err()
    assert f(ctx, _volume(fusion, buf, min_alpha=NAN), good, 1, None) == INVALID and b"min_alpha" in err()
    assert f(ctx, _volume(fusion, buf, near=INF), good, 1, None) == INVALID and b"near" in err()
    for missing in ("tsdf", "weight"):
        assert f(ctx, _volume(fusion, buf, **{missing: None}), good, 1, None) == INVALID and b"NULL tsdf or weight" in err()
    assert f(ctx, _volume(fusion, buf), views(_view(fusion, buf), _view(fusion, buf, depth=None)), 2, None) == INVALID and b"view 1 has a NULL depth" in err()
    for size in (dict(h=-1), dict(w=-1), dict(h=32769), dict(w=32769)):
        assert f(ctx, _volume(fusion, buf), views(_view(fusion, buf, **size)), 1, None) == INVALID and b"[0, 32768]" in err()
    assert f(ctx, _volume(fusion, buf), views(_view(fusion, buf, fx=NAN)), 1, None) == INVALID and b"finite" in err()
    # nothing to do is not an error: no view, or an empty volume with or without pointers
    assert f(ctx, _volume(fusion, buf), None, 0, None) == 0
    assert f(ctx, _volume(fusion, buf), good, 0, None) == 0
    assert f(ctx, _volume(fusion, buf, nx=0), good, 1, None) == 0
    assert f(ctx, _volume(fusion, buf, nz=0, tsdf=None, weight=None), good, 1, None) == 0
    assert f(ctx, _volume(fusion, buf, nx=1024, ny=1024, nz=1024), good, 0, None) == 0          # exactly the limit


def test_isosurface_refuses_bad_arguments_without_a_gpu():
    from taichi_3d_gaussian_splatting_amd import _native, fusion
    fusion._bind()
    plan, emit, err = _native.lib().gs_isosurface_plan, _native.lib().gs_isosurface_emit, _native.lib().gs_last_error
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    assert plan(None, _iso(fusion, buf), p, p, p, None) == INVALID and b"ctx is NULL" in err()
    assert emit(None, _iso(fusion, buf), p, p, p, 1, 1, p, None, p, None) == INVALID and b"ctx is NULL" in err()
    ctx = C.c_void_p(8)
    calls = (("plan", lambda vol, ws=p: plan(ctx, vol, ws, ws, p, None)), ("emit", lambda vol, ws=p: emit(ctx, vol, ws, ws, p, 1, 1, p, None, p, None)))
    for name, call in calls:
        assert call(None) == INVALID and b"volume is NULL" in err(), name
        assert call(_iso(fusion, buf, ny=-1)) == INVALID and b"dimension" in err(), name
        assert call(_iso(fusion, buf, nx=1024, ny=1024, nz=1025)) == INVALID and b"GS_FUSION_MAX_VOXELS" in err(), name
        for bad in (0.0, -1.0, NAN, INF):
            assert call(_iso(fusion, buf, spacing=_three(0.1, bad, 0.1))) == INVALID and b"spacing" in err(), name
        assert call(_iso(fusion, buf, origin=_three(INF, 0, 0))) == INVALID and b"origin" in err(), name
        assert call(_iso(fusion, buf, level=NAN)) == INVALID and b"level" in err(), name
        assert call(_iso(fusion, buf, values=None)) == INVALID and b"NULL values" in err(), name
        assert call(_iso(fusion, buf), None) == INVALID and b"NULL work buffer" in err(), name
        assert call(_iso(fusion, buf, nx=0)) == 0, name                # an empty volume has an empty mesh: no launch
        assert call(_iso(fusion, buf, nz=0, values=None), None) == 0, name
    assert plan(ctx, _iso(fusion, buf), p, p, None, None) == INVALID and b"NULL totals" in err()
    for nv, nf in ((-1, 1), (1, -1), (2 ** 31, 1), (1, 2 ** 31)):
        assert emit(ctx, _iso(fusion, buf), p, p, p, nv, nf, p, None, p, None) == INVALID and b"2^31 - 1" in err()
    assert emit(ctx, _iso(fusion, buf), p, p, None, 1, 1, p, None, p, None) == INVALID and b"NULL work buffer" in err()
    assert emit(ctx, _iso(fusion, buf), p, p, p, 1, 1, None, None, p, None) == INVALID and b"NULL vertices or faces" in err()
    assert emit(ctx, _iso(fusion, buf), p, p, p, 1, 1, p, None, None, None) == INVALID and b"NULL vertices or faces" in err()
    assert emit(ctx, _iso(fusion, buf), p, p, p, 0, 0, None, None, None, None) == 0     # nothing crosses: nothing to write


def test_macros_agree_between_the_header_and_python():
    from taichi_3d_gaussian_splatting_amd import fusion
    import fusion_ref
    assert _define("GS_TSDF_VIEWS_PER_LAUNCH") == fusion.VIEWS_PER_LAUNCH == fusion_ref.VIEWS_PER_LAUNCH == 16
    assert _define("GS_FUSION_MAX_VOXELS") == fusion.MAX_VOXELS == 2 ** 30
    assert _define("GS_FUSION_MAX_IMAGE_SIZE") == fusion.MAX_IMAGE_SIZE == 2 ** 15
    assert _define("GS_ISO_BLOCK") == fusion.ISO_BLOCK == 256
    # the launch argument (the volume and the views of one launch) fits the 4 KiB of kernel arguments
    assert C.sizeof(fusion.GsTsdfVolume) + 8 + fusion.VIEWS_PER_LAUNCH * C.sizeof(fusion.GsTsdfView) <= 4096
    # a voxel owns at most 7 crossings and a cell has at most 12 triangles: a block's sums and a round of 256 of them fit 32 bits
    assert 12 * fusion.ISO_BLOCK * fusion.ISO_BLOCK < 2 ** 32
    text = open(HEADER).read()
    for n in (1, 255, 256, 257, 48 * 40 * 36):
        for macro, fn in (("GS_ISO_CELL_WS_BYTES", fusion.cell_ws_bytes), ("GS_ISO_BLOCK_WS_BYTES", fusion.block_ws_bytes),
                          ("GS_ISO_VOXEL_WS_BYTES", fusion.voxel_ws_bytes)):
            body = re.search(r"#define %s\(n\) (.*)" % macro, text).group(1)
            expr = body.replace("(int64_t)", "").replace("GS_ISO_BLOCK", "256").replace("/", "//")
            assert eval(expr, {"n": n}) == fn(n), (macro, n)


def test_cpu_tensors_and_bad_layouts_are_refused():
    from taichi_3d_gaussian_splatting_amd import fusion
    with pytest.raises(ValueError, match="GPU"):
        fusion.isosurface(torch.zeros(4, 4, 4), (0, 0, 0), 0.1, 0.0)
    with pytest.raises(ValueError, match="GPU"):
        fusion.TSDFVolume(origin=(0, 0, 0), dims=(4, 4, 4), voxel=0.1, device="cpu")
    with pytest.raises(ValueError, match="bbox or origin"):
        fusion.TSDFVolume(dims=(4, 4, 4), voxel=0.1)


def test_world_to_camera_inverts_the_pose():
    from taichi_3d_gaussian_splatting_amd import fusion
    import fusion_ref
    rng = np.random.default_rng(3)
    q, t = rng.normal(size=4), rng.normal(size=3)
    m = fusion.world_to_camera(torch.tensor(q), t)
    assert m.dtype == np.float32 and m.shape == (3, 4) and m.tobytes() == fusion_ref.world_to_camera(q, t).tobytes()
    x, y, z, w = q / np.linalg.norm(q)
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                  [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
    p_camera = rng.normal(size=3)
    p_world = R @ p_camera + t                                      # T_pointcloud_camera takes camera coordinates to the world
    assert np.abs(m[:, :3].astype(np.float64) @ p_world + m[:, 3] - p_camera).max() < 1e-5


def test_product_sources_do_not_mention_the_checker():
    for path in (os.path.join(PKG, "fusion.py"), os.path.join(PKG, "csrc", "k_fusion.hip"), HEADER):
        assert "oracle" not in open(path).read().lower(), path
