"""CPU tests of the Python binding itself (inria_wbc_amd/capi.py): the signature table and the ctypes structures against include/wbcqp.h, the three
pointer rules, the allocator of the _host methods' outputs.  No device is needed: the header is parsed, or compiled by the host C compiler."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np

from inria_wbc_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "wbcqp.h")


def header_text() -> str:
    """include/wbcqp.h without its comments."""
    hdr = open(HEADER).read()
    return re.sub(r"//[^\n]*", " ", re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S))


def prototypes() -> dict:
    """name -> (return type, [parameter declarations]) of every function the header declares."""
    out = {}
    for ret, name, params in re.findall(r"\b(int64_t|int|const\s+char\s*\*)\s*(wbcqp_[a-z_0-9]+)\s*\(([^)]*)\)\s*;", header_text()):
        params = [" ".join(p.split()) for p in params.split(",")]
        out[name] = (" ".join(ret.split()), [] if params == ["void"] else params)
    return out


def is_pointer_type(t) -> bool:
    return t in (ctypes.c_void_p, ctypes.c_char_p) or (isinstance(t, type) and issubclass(t, ctypes._Pointer))


SCALARS = {"int": ctypes.c_int, "int32_t": ctypes.c_int32, "double": ctypes.c_double, "size_t": ctypes.c_size_t}
RETURNS = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "const char*": ctypes.c_char_p, "const char *": ctypes.c_char_p}


def test_signature_table_agrees_with_the_header(built_lib):
    assert set(capi.SIGNATURES) == set(capi.EXPORTS), set(capi.SIGNATURES) ^ set(capi.EXPORTS)
    assert len(capi.EXPORTS) == len(set(capi.EXPORTS))
    lib = capi.declare(ctypes.CDLL(built_lib))  # (a handle of its own: nothing that capi.load_library did counts)
    protos = prototypes()
    assert set(protos) == set(capi.EXPORTS), set(protos) ^ set(capi.EXPORTS)
    for name in capi.EXPORTS:
        fn = getattr(lib, name)
        ret, params = protos[name]
        assert fn.argtypes is not None, name  # (what wbcqp_launch_order, wbcqp_rollout and wbcqp_integrate_host lacked)
        assert fn.restype is RETURNS[ret], (name, ret, fn.restype)
        assert len(fn.argtypes) == len(params), (name, params, fn.argtypes)
        for decl, t in zip(params, fn.argtypes):
            if "*" in decl:
                assert is_pointer_type(t), (name, decl, t)
            else:
                ctype = " ".join(decl.split()[:-1])  # (the declaration without the parameter's name)
                assert ctype in SCALARS, (name, decl)
                assert t is SCALARS[ctype], (name, decl, t)


def structures() -> dict:
    """name -> class of every ctypes.Structure capi defines."""
    return {k: v for k, v in vars(capi).items() if isinstance(v, type) and issubclass(v, ctypes.Structure) and v.__module__ == capi.__name__}


def layout_mismatches(classes: dict, tmp_path) -> list:
    """Compiles a C program that prints sizeof and every offsetof of the header's struct behind each class and returns what differs from ctypes."""
    typedefs = {t.replace("wbcqp_", "").replace("_", ""): t for t in re.findall(r"\}\s*(wbcqp_[a-z_0-9]+)\s*;", header_text())}
    lines, want = [], {}
    for cname, cls in sorted(classes.items()):
        struct = typedefs[cname[1:].lower()]  # (CRolloutIO -> wbcqp_rollout_io: the names agree up to case and underscores)
        want[cname] = ctypes.sizeof(cls)
        lines.append('    printf("%s %%zu\\n", sizeof(%s));' % (cname, struct))
        for field in cls._fields_:
            member = "in" if (cname, field[0]) == ("CGroup", "inp") else field[0]  # (`in` is a Python keyword: the one name that differs)
            want["%s.%s" % (cname, field[0])] = getattr(cls, field[0]).offset
            lines.append('    printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (cname, field[0], struct, member))
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "wbcqp.h"\nint main(void)\n{\n%s\n    return 0;\n}\n' % "\n".join(lines))
    exe = str(tmp_path / "layout")
    cc = shutil.which("cc") or shutil.which("gcc")
    subprocess.run([cc, "-std=c99", "-I", os.path.dirname(HEADER), str(src), "-o", exe], check=True, capture_output=True, text=True)
    got = dict(ln.split() for ln in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines())
    assert set(got) == set(want)
    return [(k, want[k], int(got[k])) for k in want if want[k] != int(got[k])]


def test_structures_agree_with_the_header(tmp_path):
    classes = structures()
    assert len(classes) == 31, sorted(classes)
    assert layout_mismatches(classes, tmp_path) == []


def test_structure_check_sees_a_missing_and_a_moved_field(tmp_path):
    """The check above on two broken copies of a class: one field dropped, two fields swapped."""
    fields = list(capi.CStabInputs._fields_)
    dropped = type("CStabInputs", (ctypes.Structure,), {"_fields_": fields[:5] + fields[6:]})  # without ldp: what follows moves up
    assert layout_mismatches({"CStabInputs": dropped}, tmp_path)
    swapped = type("CTorqueMonitor", (ctypes.Structure,), {"_fields_": [capi.CTorqueMonitor._fields_[i] for i in (0, 1, 2, 3, 5, 4, 6)]})
    assert {k for k, _, _ in layout_mismatches({"CTorqueMonitor": swapped}, tmp_path)} == {"CTorqueMonitor.filter", "CTorqueMonitor.window"}


class Tensor:
    """Stands in for a device tensor: numel() and data_ptr() are all the pointer rules ask of one."""

    def __init__(self, numel: int, address: int):
        self._numel, self._address = numel, address

    def numel(self) -> int:
        return self._numel

    def data_ptr(self) -> int:
        return self._address


def test_pointer_rules():
    empty, full = Tensor(0, 0x1000), Tensor(6, 0x2000)
    # a device tensor, empty is absent
    assert capi.dev_ptr(None) is None and capi.dev_ptr(empty) is None and capi.dev_ptr(full) == 0x2000
    # a device tensor, empty is given: the library is to see it and say what is wrong with it; an int is a device address
    assert capi.dev_ptr_given(None) is None and capi.dev_ptr_given(empty) == 0x1000 and capi.dev_ptr_given(full) == 0x2000
    assert capi.dev_ptr_given(0x3008) == 0x3008
    # a host array
    a = np.arange(4.0)
    assert capi.host_ptr(None) is None and capi.host_ptr(a) == a.ctypes.data


def test_host_outputs():
    spec = {"a": ((3, 2), np.float64), "b": ((3,), np.int32), "c": ((3, 0, 4), np.float32), "d": ((3,), np.uint64), "e": ((3, 8), np.uint32)}
    res, ptrs = capi.host_outputs(spec, ("d", "a", "c"))
    assert list(res) == ["d", "a", "c"]
    for k in res:
        assert res[k].shape == spec[k][0] and res[k].dtype == spec[k][1] and not res[k].any() and res[k].flags["C_CONTIGUOUS"], k
    assert ptrs == [res["a"].ctypes.data, None, res["c"].ctypes.data, res["d"].ctypes.data, None]  # spec order; b and e were not asked for
    # where the method says so, an array without elements goes as NULL too (it is still returned)
    res, ptrs = capi.host_outputs(spec, tuple(spec), null_empty=True)
    assert list(res) == list(spec) and res["c"].shape == (3, 0, 4)
    assert ptrs == [res["a"].ctypes.data, res["b"].ctypes.data, None, res["d"].ctypes.data, res["e"].ctypes.data]
    assert capi.host_outputs(spec, ()) == ({}, [None] * 5)


def test_inputs_from_a_mapping():
    cin = capi.c_inputs({"h": 0x10, "Acop": 0x20, "w": None})
    assert [getattr(cin, k) for k in capi.FIELDS] == [0x10 if k == "h" else 0x20 if k == "Acop" else None for k in capi.FIELDS]
    assert capi.OUT_FIELDS == tuple(k for k, _ in capi.COutputs._fields_)
