"""CPU: libgsrast.so loads, exports every function include/gs_rasterizer.h declares, its structs
have the layout the ctypes binding assumes, and it refuses to work without a GPU (no fallback)."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "gs_rasterizer.h")


def _declared_functions():
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(gs_[a-z0-9_]+)\s*\(", src)))


def test_library_exports_every_declared_symbol():
    from taichi_3d_gaussian_splatting_amd import _native
    L = _native.lib()
    names = _declared_functions()
    assert len(names) >= 12
    for n in names:
        assert hasattr(L, n), f"libgsrast.so does not export {n}"
    assert sorted(_native.SYMBOLS) == names
    assert L.gs_abi_version() == _native.ABI_VERSION
    # every name gs_kernel_names() lists is a kernel that exists in the sources (its position is its timing id)
    kernels = L.gs_kernel_names().decode().split(",")
    csrc = os.path.join(ROOT, "taichi_3d_gaussian_splatting_amd", "csrc")
    text = "".join(open(os.path.join(csrc, f)).read() for f in os.listdir(csrc) if f.endswith(".hip"))
    assert len(kernels) == len(set(kernels)) == 13
    for k in kernels:
        assert re.search(r"__global__[^;{]*\b" + k + r"\s*\(", text), f"{k} is listed by gs_kernel_names() but is not a kernel"


# every struct of the header that the binding mirrors -> its ctypes class in _native (gs_density_scene has gs_scene's layout and class)
HEADER_STRUCTS = {"gs_config": "GsConfig", "gs_scene": "GsScene", "gs_density_scene": "GsScene", "gs_camera": "GsCamera",
                  "gs_forward_out": "GsForwardOut", "gs_frame_info": "GsFrameInfo", "gs_loss_image": "GsLossImage",
                  "gs_controller_accumulators": "GsControllerAccumulators", "gs_backward_out": "GsBackwardOut",
                  "gs_backward_extra": "GsBackwardExtra", "gs_density_config": "GsDensityConfig", "gs_density_plan": "GsDensityPlan"}
HEADER_CONSTANTS = ["GS_X_COUNT_", "GS_DENSITY_FLOATER", "GS_DENSITY_TRANSPARENT", "GS_DENSITY_DENSIFY", "GS_DENSITY_OVER",
                    "GS_DENSITY_CAM_FLOATER", "GS_DENSITY_CAM_SINGLE", "GS_DENSITY_CAM_VIEWSPACE", "GS_DC_COUNT_", "GS_ABI_VERSION"]


def _probe(tmp_path, structs, constants):
    """Compile a program against the real header with gcc (it is plain C); -> {"name": sizeof, "name.field": offsetof,
    "CONSTANT": value} for structs = {header struct name: [field names]}."""
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', 'int main(void){']
    for cname, fields in structs.items():
        lines.append(f'printf("{cname} %zu\\n", sizeof({cname}));')
        lines += [f'printf("{cname}.{f} %zu\\n", offsetof({cname}, {f}));' for f in fields]
    lines += [f'printf("{name} %d\\n", (int){name});' for name in constants]
    lines.append("return 0; }")
    src, exe = tmp_path / "probe.c", tmp_path / "probe"
    src.write_text("\n".join(lines))
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", str(src), "-o", str(exe)])
    return {k: int(v) for k, v in (l.split() for l in subprocess.check_output([str(exe)]).decode().splitlines())}


def test_struct_layouts_match_the_header(tmp_path):
    """sizeof / offsetof of every header struct against EVERY ctypes.Structure of the binding, and the header's constants."""
    from taichi_3d_gaussian_splatting_amd import _native
    mirrors = {n for n, v in vars(_native).items() if isinstance(v, type) and issubclass(v, C.Structure)}
    assert mirrors == set(HEADER_STRUCTS.values())              # a struct added to the binding has to be named above
    structs = {cname: getattr(_native, n) for cname, n in HEADER_STRUCTS.items()}
    got = _probe(tmp_path, {cname: [f for f, _ in cls._fields_] for cname, cls in structs.items()}, HEADER_CONSTANTS)
    for cname, cls in structs.items():
        assert got[cname] == C.sizeof(cls), cname
        # every field of the header struct is mirrored, in order
        for fname, _ in cls._fields_:
            assert got[f"{cname}.{fname}"] == getattr(cls, fname).offset, f"{cname}.{fname}"
    assert [f for f, _ in _native.GsBackwardExtra._fields_] == ["grad_rasterized_depth", "rasterized_depth", "grad_pixel_accumulated_alpha"]
    assert got["GS_X_COUNT_"] == len(_native.EXPORTS)
    assert got["GS_DENSITY_FLOATER"] == _native.DENSITY_FLOATER
    assert got["GS_DENSITY_TRANSPARENT"] == _native.DENSITY_TRANSPARENT
    assert got["GS_DENSITY_DENSIFY"] == _native.DENSITY_DENSIFY
    assert got["GS_DENSITY_OVER"] == _native.DENSITY_OVER
    assert got["GS_DENSITY_CAM_FLOATER"] == _native.DENSITY_CAM_FLOATER
    assert got["GS_DENSITY_CAM_SINGLE"] == _native.DENSITY_CAM_SINGLE
    assert got["GS_DENSITY_CAM_VIEWSPACE"] == _native.DENSITY_CAM_VIEWSPACE
    assert got["GS_DC_COUNT_"] == len(_native.DENSITY_COUNTS)
    assert got["GS_ABI_VERSION"] == _native.ABI_VERSION == 9


def _header_prototypes():
    """{function name: (return type, [parameter types])} of include/gs_rasterizer.h, types as written minus `const` and spaces."""
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    src = src[src.index("gs_abi_version") - 4:]                  # the prototypes follow the typedefs they use
    ctype = lambda decl: re.sub(r"\bconst\b|\s", "", decl)
    protos = {}
    for ret, name, params in re.findall(r"([A-Za-z_][\w ]*?[\w*])\s+(gs_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", src):
        params = [] if params.strip() == "void" else [re.match(r"(.*?)(\w+)$", p.strip()).group(1) for p in params.split(",")]
        protos[name] = (ctype(ret), [ctype(p) for p in params])
    return protos


def _c_kind(t):
    """The kind of a C type of the header: i32 / i64 / f32, ptr:<struct> for a mirrored struct, ptrptr, ptr, or str (char*)."""
    if t in ("int", "int32_t", "uint32_t", "gs_export"):
        return "i32"
    if t in ("int64_t", "uint64_t"):
        return "i64"
    if t == "float":
        return "f32"
    if t == "char*":
        return "str"
    if t.endswith("**"):
        return "ptrptr"
    assert t.endswith("*") or t == "gs_stream", t
    return f"ptr:{HEADER_STRUCTS[t[:-1]]}" if t[:-1] in HEADER_STRUCTS else "ptr"


def _ctypes_kind(t):
    """The same classification of a ctypes type of the binding."""
    if issubclass(t, C._Pointer):
        if issubclass(t._type_, C.Structure):
            return f"ptr:{t._type_.__name__}"
        return "ptrptr" if t._type_ is C.c_void_p else "ptr"
    code = t._type_
    if code in "iIlLqQ":
        return f"i{8 * C.sizeof(t)}"
    return {"f": "f32", "P": "ptr", "z": "str"}[code]


def test_argtypes_match_the_prototypes():
    """Every hand-written argtypes / restype of _native.lib() against the prototype in the header: the number of arguments, the
    kind of each and of the return value.  (A function the binding leaves without argtypes must take none; without a restype
    it returns ctypes' default, int.)"""
    from taichi_3d_gaussian_splatting_amd import _native
    L = _native.lib()
    protos = _header_prototypes()
    assert sorted(protos) == _declared_functions() and len(protos) == 33
    for name, (ret, params) in protos.items():
        fn = getattr(L, name)
        assert [_ctypes_kind(t) for t in fn.argtypes or ()] == [_c_kind(p) for p in params], name
        assert _ctypes_kind(fn.restype) == _c_kind(ret), name
    # _native.call() appends the stream to exactly the status-returning calls that end in one
    status_calls = {n for n, (ret, _) in protos.items() if ret == "int" and n != "gs_abi_version"}
    assert _native._STREAMLESS == {n for n in status_calls if protos[n][1][-1] != "gs_stream"}


def test_no_fallback_without_gpu():
    """On a box without a GPU the library reports an error; nothing silently runs on the CPU."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from taichi_3d_gaussian_splatting_amd import _native
    L = _native.lib()
    h = C.c_void_p()
    rc = L.gs_create(0, C.byref(h))
    assert rc < 0 and b"hip" in L.gs_last_error().lower()


def test_product_never_touches_the_oracle():
    """The shipped package must not import, link or mention oracle/ (it is test infrastructure)."""
    pkg = os.path.join(ROOT, "taichi_3d_gaussian_splatting_amd")
    for dirpath, _, files in os.walk(pkg):
        for fn in files:
            if fn.endswith((".py", ".hip", ".h", ".cpp", "Makefile")):
                text = open(os.path.join(dirpath, fn), errors="ignore").read()
                assert "gs_oracle" not in text and "from oracle" not in text and "import oracle" not in text, fn
    out = subprocess.check_output(["ldd", os.path.join(pkg, "lib", "libgsrast.so")]).decode()
    assert "gsoracle" not in out and "torch" not in out


def test_missing_library_fails_loudly(monkeypatch):
    from taichi_3d_gaussian_splatting_amd import _native
    monkeypatch.setattr(_native, "_lib", None)
    monkeypatch.setattr(_native, "LIB_PATH", "/nonexistent/libgsrast.so")
    with pytest.raises(_native.NativeLibraryError):
        _native.lib()
