"""CPU checks of the drop-in boundary: the C-ABI library builds, loads and exports every symbol
include/fluidx_hip.h declares; without a GPU the product fails loudly instead of falling back."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_functions():
    src = open(os.path.join(ROOT, "include", "fluidx_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(fx_[a-z0-9_]+)\s*\(", src)))


def test_header_declares_the_operator_surface():
    names = header_functions()
    for need in ("fx_create", "fx_destroy", "fx_set_max_samples", "fx_set_sh", "fx_update_frame", "fx_simulate",
                 "fx_render", "fx_sh_transform", "fx_upload", "fx_download", "fx_comm_init_rank"):
        assert need in names


def test_library_exports_every_declared_symbol():
    from fluidx12_amd import capi
    lib = capi.load()
    names = header_functions()
    assert set(names) == set(capi.SYMBOLS), "capi.SYMBOLS and include/fluidx_hip.h disagree"
    for n in names:
        assert hasattr(lib, n), n
    assert lib.fx_abi_version() == capi.ABI_VERSION == 7
    assert lib.fx_error_string(-6).decode().startswith("advection")


def test_no_torch_types_in_the_abi():
    src = open(os.path.join(ROOT, "include", "fluidx_hip.h")).read()
    assert "torch" not in src and "at::" not in src and "#include <hip" not in src


def test_product_does_not_reference_the_oracle():
    pkg = os.path.join(ROOT, "fluidx12_amd")
    for dp, _, fns in os.walk(pkg):
        if os.path.basename(dp) == "build":
            continue
        for fn in fns:
            if fn.endswith((".py", ".cpp", ".hip", ".h")):
                txt = open(os.path.join(dp, fn)).read()
                for line in txt.splitlines():
                    code = line.split("//")[0].split("#")[0] if not fn.endswith(".py") else line.split("#")[0]
                    assert "liborc" not in code and "fx_oracle.h" not in code, (fn, line)
                    assert not re.search(r"^\s*(from|import)\s+oracle", code), (fn, line)


def _have_gpu():
    try:
        import torch
        return torch.cuda.device_count() > 0
    except Exception:
        return os.path.exists("/dev/kfd")


@pytest.mark.skipif(_have_gpu(), reason="checks the no-GPU failure mode")
def test_create_fails_loudly_without_gpu():
    import fluidx12_amd as fx
    from fluidx12_amd import capi
    f = fx.Fluid()
    assert f.Init(800, 800, (32, 32, 32)) is False          # the reference's Init also reports failure as false
    assert f.last_status == capi.FX_E_DEVICE
    with pytest.raises(fx.FluidxError):
        f.Simulate(0)


def test_create_rejects_bad_descriptors():
    from fluidx12_amd import capi
    lib = capi.load()
    ctx = C.c_void_p()
    d = capi.Desc()
    assert lib.fx_create(C.byref(ctx), C.byref(d)) == capi.FX_E_INVALID      # struct_size 0
    d.struct_size = C.sizeof(capi.Desc)
    d.grid_x, d.grid_y, d.grid_z, d.jacobi_iters = 32, 16, 8, 4              # x != y (Fluid.cpp:201)
    assert lib.fx_create(C.byref(ctx), C.byref(d)) == capi.FX_E_INVALID
    assert lib.fx_destroy(None) == capi.FX_E_INVALID


def test_header_is_plain_c99_and_cxx11(tmp_path):
    """the boundary is a C ABI: the header must compile as C99 and as C++11 on its own (no HIP, no torch, no C++-only syntax)"""
    import shutil
    import subprocess
    src = tmp_path / "abi_probe.c"
    src.write_text('#include "fluidx_hip.h"\nint main(void) { fx_desc d; fx_frame_info fi; fx_timing t; d.struct_size = sizeof d;\n'
                   '  (void)fi; (void)t; return FX_ABI_VERSION > 0 && FX_OPT_OVERLAP == 1 ? 0 : 1; }\n')
    inc = os.path.join(ROOT, "include")
    if shutil.which("gcc"):
        subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only", "-I", inc, str(src)], check=True)
    if shutil.which("g++"):
        subprocess.run(["g++", "-std=c++11", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", inc, "-x", "c++", str(src)], check=True)


def test_cxx_shim_and_demo_compile():
    """the C++ mirror of class Fluid (csrc/Fluid.hpp) and the demo driver build against the header with a host compiler
    (syntax only: linking needs the HIP runtime)"""
    import shutil
    import subprocess
    if not shutil.which("g++"):
        pytest.skip("no g++")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-fsyntax-only", os.path.join(ROOT, "examples", "fluidx_demo.cpp")], check=True)


def test_the_shipped_library_offers_ten_switches():
    """lab equipment stays in the lab.  fx_knob_name enumerates at most ten names in the shipped build -- switches a
    caller could need -- and fx_set_knob refuses every other name (the launchers then run on their defaults); the A/B switches of the
    launchers and the superseded kernels behind them exist with -DFX_LAB only"""
    from fluidx12_amd import build, capi
    names = capi.knob_names()
    if build.LAB:
        assert len(names) > 40 and "STRIP4_OCTET" in names
        return
    assert names == sorted(names) and len(names) <= 10, names
    assert "ADVECT_LDS" in names and "JACOBI_T" in names
    assert capi.load().fx_set_knob(b"STRIP4_OCTET", b"0") == capi.FX_E_INVALID
    import subprocess
    syms = subprocess.run(["nm", "-D", "--defined-only", build.LIB], capture_output=True, text=True, check=True).stdout
    assert "k_jacobi_strip4q" not in syms
