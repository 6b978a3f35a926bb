"""The C-ABI library loads and exports every symbol include/tapqir_hip.h declares (no GPU needed)."""

import ctypes
import os
import re

import pytest

from tapqir_amd import _lib
from tapqir_amd.exceptions import HipExtensionError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols():
    text = open(os.path.join(ROOT, "include", "tapqir_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(tq_[a-z_0-9]+)\s*\(", text)))


def test_header_and_binding_agree():
    assert declared_symbols() == sorted(_lib.EXPORTS)


def test_library_exports_every_declared_symbol():
    from tapqir_amd.build import build

    build(verbose=False)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in declared_symbols():
        assert hasattr(lib, name), name
    assert _lib.load().tq_version() >= 100


# the ctypes mirrors of the header's argument structs: {C name (from the mirror's docstring): class}
MIRRORS = {re.search(r"``(tq_\w+)``", c.__doc__).group(1): c for c in vars(_lib).values()
           if isinstance(c, type) and issubclass(c, ctypes.Structure) and c is not ctypes.Structure}


def header_fields(name):
    """Field names of ``typedef struct { ... } name;`` in include/tapqir_hip.h, in order."""
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tapqir_hip.h")).read(), flags=re.S)
    body = re.search(r"typedef struct \{([^{}]*)\}\s*%s;" % name, text).group(1)
    out = []
    for decl in body.split(";"):
        if decl.strip():  # "const float* p" | "int32_t P, K, O" | "double lamda_g[4]": the declarators' identifiers
            first, *more = decl.split(",")
            out += [re.search(r"(\w+)\s*(\[[^\]]*\]\s*)*$", d.strip()).group(1) for d in [first] + more]
    return out


def test_struct_sizes_match_the_c_header():
    """ctypes mirrors of the argument structs have the C compiler's layout: sizeof and the offsetof of EVERY field of all
    twelve, the C generated from each mirror's _fields_; and a mirror names the fields the header declares, in its order (a
    field added at the end of the C struct can hide in the tail padding, where neither size nor offsets show it)."""
    import subprocess
    import tempfile

    assert len(MIRRORS) == 12 and {"tq_rsample_args", "tq_snr_args", "tq_cosmos_args", "tq_ksmogn_args"} <= set(MIRRORS)
    lines, want = [], []
    for cname, cls in sorted(MIRRORS.items()):
        names = [f[0] for f in cls._fields_]
        assert names == header_fields(cname), cname
        lines.append('  printf("%%zu\\n", sizeof(%s));' % cname)
        want.append((cname, "sizeof", ctypes.sizeof(cls)))
        for f in names:
            lines.append('  printf("%%zu\\n", offsetof(%s, %s));' % (cname, f))
            want.append((cname, f, getattr(cls, f).offset))
    head = '#include <stdio.h>\n#include <stddef.h>\n#include "tapqir_hip.h"\nint main(void) {\n'
    src = head + "\n".join(lines) + "\n  return 0;\n}\n"
    with tempfile.TemporaryDirectory() as td:
        c = os.path.join(td, "s.c")
        open(c, "w").write(src)
        exe = os.path.join(td, "s")
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        got = [int(v) for v in subprocess.check_output([exe]).split()]
    assert len(got) == len(want)
    assert [(n, f, g) for (n, f, _), g in zip(want, got)] == want


# the constants of the header that the binding mirrors: every upper-case integer of tapqir_amd._lib
MIRRORED = sorted(n for n, v in vars(_lib).items() if n.isupper() and type(v) is int)


@pytest.mark.parametrize("name", MIRRORED)
def test_mirrored_constants_match_the_c_header(name):
    text = open(os.path.join(ROOT, "include", "tapqir_hip.h")).read()
    found = re.findall(r"^#define TQ_%s\s+(\d+)\b" % name, text, flags=re.M)
    assert len(found) == 1, "TQ_%s is not #defined (once, as an integer) in include/tapqir_hip.h" % name
    assert int(found[0]) == getattr(_lib, name)


def test_the_engine_constants_are_mirrored():
    assert {"TAIL_ROWS16", "PIXEL_FUSED_UNIT", "SYNC_WORDS", "SUBSAMPLE_MAX", "GSUM_LEN"} <= set(MIRRORED)


def test_argument_validation_returns_error_codes_without_a_gpu():
    lib = _lib.load()
    a = _lib.KsmognArgs()
    assert lib.tq_ksmogn_log_prob(ctypes.byref(a), None) == 1  # TQ_ERR_ARG
    assert b"NULL" in lib.tq_last_error()
    c = _lib.CosmosArgs()
    assert lib.tq_cosmos_step(ctypes.byref(c), None) == 1


def test_no_cpu_fallback():
    """The product refuses to run the SVI step anywhere but on the HIP device."""
    from tapqir_amd.models.cosmos import cosmos
    from tapqir_amd.utils.simulate import TEST_PARAMS, simulate

    m = cosmos(device="cpu")
    m.data = simulate(m, 2, 3, 1, 14, 0, TEST_PARAMS)
    with pytest.raises(HipExtensionError):
        m.init()


def test_missing_library_fails_loudly(monkeypatch, tmp_path):
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "LIB_PATH", str(tmp_path / "nope.so"))
    with pytest.raises(HipExtensionError):
        _lib.load()
