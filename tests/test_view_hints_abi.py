"""CPU: the C ABI of the view table's read-out (include/gs_view_hints.h)."""
import ctypes as C
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "gs_view_hints.h")
INVALID = -1                                                      # GS_ERR_INVALID_ARGUMENT


def test_header_is_plain_c99_and_declares_the_one_function(tmp_path):
    src = tmp_path / "probe.c"
    src.write_text(f'#include "{HEADER}"\n'
                   'int main(void) {\n'
                   '  int (*f)(gs_ctx*, const gs_frame*, int32_t, int32_t*, int32_t*, float*, int32_t*, int32_t, int32_t*, int32_t,\n'
                   '           int32_t*) = gs_view_hints_read;\n'
                   '  (void)f; return GS_VIEW_KEY_FLOATS == 7 ? 0 : 1; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-c", str(src), "-o", str(tmp_path / "probe.o")])


def test_library_exports_the_symbol_and_the_main_header_is_unchanged():
    from taichi_3d_gaussian_splatting_amd import _native
    L = _native.lib()
    assert hasattr(L, "gs_view_hints_read") and "gs_view_hints_read" not in _native.SYMBOLS
    assert L.gs_abi_version() == _native.ABI_VERSION == 9
    assert "view_hints" not in open(os.path.join(ROOT, "include", "gs_rasterizer.h")).read().lower()


def test_refuses_bad_arguments_without_a_gpu():
    from taichi_3d_gaussian_splatting_amd import _native
    L = _native.lib()
    f = L.gs_view_hints_read
    I32P = C.POINTER(C.c_int32)
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, I32P, I32P, C.POINTER(C.c_float), I32P, C.c_int32, I32P, C.c_int32, I32P]
    f.restype = C.c_int
    L.gs_last_error.restype = C.c_char_p
    assert f(None, None, -1, None, None, None, None, 0, None, 0, None) == INVALID and b"ctx is NULL" in L.gs_last_error()
