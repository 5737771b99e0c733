import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with -m gpu on the GPU box)")


def _have_gpu():
    # device_count() does not initialise the GPU on this image
    try:
        import torch
        return torch.cuda.device_count() > 0
    except Exception:
        return os.path.exists("/dev/kfd")


def pytest_collection_modifyitems(config, items):
    if _have_gpu():
        return
    skip = pytest.mark.skip(reason="no GPU in this container")
    for it in items:
        if "gpu" in it.keywords:
            it.add_marker(skip)


LAB_LIB = os.path.join(ROOT, "tools", "_variants", "libfluidx_hip_lab.so")
_lab = []


def lab_library():
    """the lab build of the library (-DFX_LAB, built by __graft_entry__.build(); here on demand if missing), opened beside the shipped one:
    RTLD_LOCAL keeps its symbols out of the shipped library's way, RTLD_DEEPBIND binds its own calls to its own definitions"""
    if not _lab:
        import ctypes
        from fluidx12_amd import build, capi
        if not os.path.exists(LAB_LIB) or os.path.getmtime(LAB_LIB) < os.path.getmtime(build.ensure_built()):
            build.build_variant("lab", ["-DFX_LAB"], sources=build.lab_sources())
        lib = ctypes.CDLL(LAB_LIB, mode=os.RTLD_LOCAL | os.RTLD_DEEPBIND)
        lib.fx_abi_version.restype, lib.fx_abi_version.argtypes = ctypes.c_int, []
        assert lib.fx_abi_version() == capi.ABI_VERSION, LAB_LIB
        for name, (res, args) in capi.SYMBOLS.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        _lab.append(lib)
    return _lab[0]


@pytest.fixture
def knob(monkeypatch):
    """sets measurement switches of the kernel launchers for one test (fx_set_knob: which kernel of the library serves a geometry);
    usage: knob("ADVECT_LDS", "0"); every switch touched goes back to its default behind the test.  The shipped library offers ten
    switches; the launchers' A/B switches (and the superseded kernels behind some of them) exist in the lab build only.  The first lab switch
    a test sets moves it onto the lab build: the switches it set before are set there too, the contexts it creates from then on and the
    helpers and child processes that open the library by path (FLUIDX_LIB_PATH) use it.  Contexts created before stay on the shipped
    library, with the switches that were set when they were created."""
    from fluidx12_amd import capi
    touched = []                                    # (library, name, value) in the order set

    def setter(name, value):
        if name not in capi.knob_names():          # a lab switch (on the lab build already: set_knob below refuses an unknown name)
            lab = lab_library()
            if capi.load() is not lab:
                monkeypatch.setattr(capi, "_lib", lab)
                monkeypatch.setenv("FLUIDX_LIB_PATH", LAB_LIB)
                for _, n, v in list(touched):
                    capi.set_knob(n, v)
                    touched.append((lab, n, v))
        capi.set_knob(name, value)
        touched.append((capi.load(), name, value))

    yield setter
    for lib, name, _ in reversed(touched):
        capi.check(lib.fx_set_knob(name.encode(), None), "set_knob(%s)" % name)
