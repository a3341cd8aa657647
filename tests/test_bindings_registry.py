"""The registry of extension headers (fountain_amd/_abi.py EXTENSIONS) and the binder over it (fountain_amd/_nontwin.py bind) without a
GPU: for every extension the header, the prototype table and the library's exports agree -- names, arity and which functions return
nothing, and the kind of every argument --; no function belongs to two tables; no header under include/ lacks an entry; bind applies the
prototypes once per library and makes both refusals with their texts."""
import ctypes as C
import glob
import os
import re

import pytest

from fountain_amd import _abi as A
from fountain_amd._nontwin import bind

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")


def kinds(param):
    """the ctypes a table may hold for one parameter of a declaration: pointers and arrays are c_void_p (a string may be c_char_p, a
    pointer to pointers a POINTER type), scalars exactly their C type"""
    if "*" in param or "[" in param:
        if param.count("*") > 1 or "[" in param and "*" in param:
            return None                                                 # any pointer type
        return (C.c_void_p, C.c_char_p) if re.match(r"\s*const\s+char\s*\*", param) else (C.c_void_p,)
    scalar = re.match(r"\s*(?:const\s+)?(\w+)\s+\w+\s*$", param).group(1)
    return ({"int": C.c_int, "int32_t": C.c_int32, "uint32_t": C.c_uint32, "size_t": C.c_size_t, "float": C.c_float}[scalar],)


def declarations(header):
    """{function: (result type, the parameters' texts)} of a header's ftn_* declarations, comments stripped"""
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(INCLUDE, header)).read(), flags=re.S)
    out = {}
    for result, name, args in re.findall(r"([A-Za-z_][\w \t]*?[\w*])\s*\b(ftn_[a-z0-9_]+)\s*\((.*?)\)\s*;", src, re.S):
        assert name not in out, "%s declares %s twice" % (header, name)
        out[name] = (" ".join(result.split()), [] if args.strip() == "void" else args.split(","))
    assert sorted(out) == sorted(set(re.findall(r"\b(ftn_[a-z0-9_]+)\s*\(", src))), header       # (the names as the per-extension ABI tests find them)
    return out


@pytest.mark.parametrize("key", sorted(A.EXTENSIONS))
def test_header_table_and_exports_agree(ftn, key):
    ext = A.EXTENSIONS[key]
    assert ext.header == "fountain_hip_%s.h" % key and os.path.exists(os.path.join(INCLUDE, ext.header))
    declared = declarations(ext.header)
    assert sorted(declared) == sorted(ext.prototypes) == getattr(A, key.upper() + "_FUNCTIONS")
    assert ext.abi_version_fn in declared
    for name, (argtypes, restype) in ext.prototypes.items():
        result, params = declared[name]
        assert len(params) == len(argtypes), name
        for param, argtype in zip(params, argtypes):
            allowed = kinds(param)
            assert argtype in allowed if allowed else issubclass(argtype, (C._Pointer, C.c_void_p)), "%s: %s is %s" % (name, param.strip(), argtype)
        assert (restype is None) == (result == "void"), name
        assert hasattr(ftn.lib, name), "libfountain_hip.so does not export %s" % name


def test_no_function_is_listed_twice():
    seen = {name: "DECLARED_FUNCTIONS" for name in A.DECLARED_FUNCTIONS}
    assert len(seen) == len(A.DECLARED_FUNCTIONS)
    for key, ext in A.EXTENSIONS.items():
        for name in ext.prototypes:
            assert name not in seen, "%s is listed by %s and by %s" % (name, seen[name], key)
            seen[name] = key


def test_every_extension_header_is_registered():
    headers = sorted(os.path.basename(p) for p in glob.glob(os.path.join(INCLUDE, "fountain_hip_*.h")))
    assert headers == sorted(ext.header for ext in A.EXTENSIONS.values())
    tables = sorted(name for name in dir(A) if name.endswith("_PROTOTYPES") and name != "CORE_PROTOTYPES")
    assert tables == sorted(key.upper() + "_PROTOTYPES" for key in A.EXTENSIONS)
    assert all(getattr(A, key.upper() + "_PROTOTYPES") is ext.prototypes for key, ext in A.EXTENSIONS.items())


def test_core_prototypes_are_functions_of_the_core_header(ftn):
    assert set(A.CORE_TWINS) <= set(A.CORE_PROTOTYPES)
    declared = declarations("fountain_hip.h")
    for name, (argtypes, restype) in A.CORE_PROTOTYPES.items():
        result, params = declared["ftn_" + name]
        assert "ftn_" + name in A.DECLARED_FUNCTIONS
        assert argtypes is None or len(params) == len(argtypes), name
        for param, argtype in zip(params, argtypes or ()):
            allowed = kinds(param)
            assert argtype in allowed if allowed else issubclass(argtype, (C._Pointer, C.c_void_p)), "%s: %s is %s" % (name, param.strip(), argtype)
        assert (restype is None) == (result == "void"), name
        assert getattr(ftn.lib, "ftn_" + name).restype is restype, name
    for name, argtypes in (("interaction", A.TEST_INTERACTION_ARGTYPES), ("camera", A.TEST_CAMERA_ARGTYPES)):
        assert A.CORE_PROTOTYPES["test_" + name][0] is argtypes


def test_bind_applies_the_prototypes_once(ftn):
    for ext in A.EXTENSIONS.values():
        assert bind(ftn, ext) is ftn.lib and ext.header in ftn.bound
        first = {name: getattr(ftn.lib, name).argtypes for name in ext.prototypes}
        for name, (argtypes, restype) in ext.prototypes.items():
            assert list(first[name]) == list(argtypes) and getattr(ftn.lib, name).restype is restype, name
        assert bind(ftn, ext) is ftn.lib
        for name in ext.prototypes:
            assert getattr(ftn.lib, name).argtypes is first[name], name
        # the table's own lists would be the same objects after a second application too: an equal list put in their place must survive
        probe = getattr(ftn.lib, ext.abi_version_fn)
        probe.argtypes = marker = list(first[ext.abi_version_fn])
        try:
            assert bind(ftn, ext) is ftn.lib and probe.argtypes is marker, ext.header
        finally:
            probe.argtypes = first[ext.abi_version_fn]


def test_bind_refuses_the_oracle_with_the_extensions_sentence(orc):
    from fountain_amd import FountainError
    for key, ext in A.EXTENSIONS.items():
        with pytest.raises(FountainError) as e:
            bind(orc, ext)
        assert e.value.code == A.FTN_ERR_UNSUPPORTED and str(e.value).endswith(": " + ext.no_twin), key
    assert not orc.bound


class _OtherVersion:
    """a stand-in for a loaded library whose every ftn_*_abi_version reports 7"""

    def __getattr__(self, name):
        if not name.endswith("_abi_version"):
            raise AttributeError(name)
        return lambda: 7


def test_bind_refuses_another_abi_version_with_its_text():
    from fountain_amd import FountainError

    class Stub:
        lib, path, is_oracle = _OtherVersion(), "/somewhere/libfountain_hip.so", False

    for key, ext in A.EXTENSIONS.items():
        be = Stub()
        be.bound = set()
        for _ in range(2):                      # a refusal is not remembered as a success
            with pytest.raises(FountainError) as e:
                bind(be, ext)
            assert e.value.code == A.FTN_ERR_INTERNAL and not be.bound
            assert str(e.value) == ("fountain error -7: /somewhere/libfountain_hip.so reports %s ABI version 7, this binding was written for %d: "
                                    "rebuild the library" % (ext.what, ext.abi_version)), key
    whats = {key: ext.what for key, ext in A.EXTENSIONS.items()}
    assert whats == {"gbuffer": "G-buffer", "denoise": "denoise", "denoise_guided": "guided denoise", "moments": "moments", "adaptive": "adaptive",
                     "temporal": "temporal", "filter": "filter", "display": "display", "bloom": "bloom", "vectorblur": "vector-blur",
                     "metrics": "metrics", "subdiv": "subdivision", "idmatte": "ID-matte", "ao": "ambient-occlusion", "lightpass": "light-pass",
                     "motion": "motion"}
