"""No GPU: the stream entries of the C ABI as the header declares them, what they answer without a device, and the Python front's
two switches (api.use_torch_stream / api.use_own_stream).  The ordering itself is tests/test_gpu_streams.py's."""
import ctypes as C
import os
import re

import pytest

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "lcg_hip.h")
CTYPE = {"int": C.c_int, "void *": C.c_void_p, "void": None}


def _prototype(name):
    """(return type, [argument types]) of `name` as the header spells them, comments removed."""
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"^\s*([a-z_ ]+?\*?)\s*" + name + r"\s*\(([^)]*)\)\s*;", src, flags=re.M)
    assert m, name
    ret = m.group(1).strip()
    ret = "void *" if ret.replace(" ", "") == "void*" else ret
    args = [a.strip() for a in m.group(2).split(",")]
    args = [] if args == ["void"] else ["void *" if "*" in a else a.split()[0] for a in args]
    return ret, args


def test_prototypes_match_the_header():
    from liblcg_amd import _lib
    assert _prototype("lcg_hip_set_stream") == ("int", ["void *"])
    assert _prototype("lcg_hip_get_stream") == ("void *", [])
    for name in ("lcg_hip_set_stream", "lcg_hip_get_stream"):
        ret, args = _prototype(name)
        assert _lib.SIGNATURES[name] == (CTYPE[ret], [CTYPE[a] for a in args]), (name, _lib.SIGNATURES[name])


def test_the_header_and_the_guide_state_both_rules():
    """The contract next to the prototype and in INTEGRATION.md: the new stream waits for the previous one; the previous one must
    still exist."""
    src = open(HEADER).read()
    at = src.index("int  lcg_hip_set_stream(")
    note = " ".join(src[max(0, at - 1200):at].split())
    assert "waits" in note and "previous stream" in note and "must still exist" in note and "does nothing" in note, note
    guide = " ".join(open(os.path.join(ROOT, "INTEGRATION.md")).read().split())
    assert "lcg_hip_set_stream" in guide and "must still exist" in guide and "waits" in guide


def test_without_a_device_the_entries_say_so():
    import torch
    from liblcg_amd import _lib
    lib = _lib.load()
    if torch.cuda.is_available():
        pytest.skip("GPU present: the no-device path cannot be exercised")
    assert lib.lcg_hip_set_stream(None) == -2001                # LCG_HIP_E_NO_DEVICE
    assert lib.lcg_hip_set_stream(C.c_void_p(1)) == -2001
    assert b"no" in lib.lcg_hip_last_error().lower()
    assert lib.lcg_hip_get_stream() is None                     # NULL
    assert lib.lcg_hip_synchronize() == -2001


def test_the_python_front_has_both_switches():
    import torch
    from liblcg_amd import api
    assert callable(api.use_own_stream) and callable(api.use_torch_stream)
    if not torch.cuda.is_available():
        with pytest.raises(api.LcgHipError):                    # a missing device is an error, not a silent no-op
            api.use_own_stream()
