"""CPU tests of the drop-in boundary: the C-ABI library loads, exports every symbol the
header declares, validates arguments, and the host mirror keeps the reference's error
behaviour.  No compute is attempted without a GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT


def header_symbols():
    text = open(os.path.join(ROOT, "include", "dq_sufsort.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(dq_[a-z0-9_]+)\s*\(", text)))


def test_library_exports_every_declared_symbol(backend_lib):
    from deltaq_amd import _abi
    syms = header_symbols()
    assert set(syms) == set(_abi.EXPORTS)
    for s in syms:
        assert hasattr(backend_lib, s), f"{s} declared in include/dq_sufsort.h but not exported"


def test_abi_version(backend_lib):
    assert backend_lib.dq_abi_version() == 1
    assert backend_lib.dq_device_count() >= 0


def test_workspace_query(backend_lib):
    n = 1 << 20
    b4 = backend_lib.dq_sufsort_hip_workspace_bytes(n, 4)
    b8 = backend_lib.dq_sufsort_hip_workspace_bytes(n, 8)
    assert 40 * n <= b4 < 41 * n + (16 << 20)      # 28 B/byte + the third list buffer (12 B/byte, round 5) + fixed tables
    assert 52 * n <= b8 < 53 * n + (16 << 20)      # 36 + 16
    assert backend_lib.dq_sufsort_hip_workspace_bytes(n, 3) == -1
    assert backend_lib.dq_sufsort_hip_workspace_bytes(-5, 4) == -1
    # int64 on both sides of 2^32: 59 B per byte with the third list buffer (X, Xs) just below, 43 B at exactly 2^32,
    # which never carves it
    below, at = (1 << 32) - 1, 1 << 32
    assert 59 * below <= backend_lib.dq_sufsort_hip_workspace_bytes(below, 8) < 59.05 * below
    assert 43 * at <= backend_lib.dq_sufsort_hip_workspace_bytes(at, 8) < 43.05 * at
    assert 47 * INT_MAX <= backend_lib.dq_sufsort_hip_workspace_bytes(INT_MAX, 4) < 47.05 * INT_MAX


INT_MAX = (1 << 31) - 1
HBM = 288 * 10**9 - (2 << 30)          # an MI355X (288 GB) less 2 GiB for the runtime and whatever else is resident


def test_workspace_plan_fits_every_length(backend_lib):
    """The layout a sort carves is chosen from what fits (dq_sufsort_hip_workspace_plan, the host function the entry
    points call with the device's free memory): the full layout where it fits, otherwise the one without the third
    list buffer.  For every n the 64-bit contract accepts, and every int32 n, the chosen workspace plus the caller's
    device buffers must fit one MI355X -- through the host entry (workspace + the device copy of sa) and through the
    device entry (workspace + the caller's text and sa)."""
    plan = backend_lib.dq_sufsort_hip_workspace_plan
    lengths = sorted({(1 << 31) + 1, 3 << 30, 4_030_000_000, 4_200_000_000, (1 << 32) - 1, 1 << 32} |
                     {int(x) for x in np.linspace(1 << 20, 1 << 32, 4097)})
    for n in lengths:
        for wb, host in ((8, 1), (8, 0), (4, 1), (4, 0)):
            if wb == 4 and n > INT_MAX:
                continue
            caller = 0 if host else n + wb * n
            avail = HBM - caller
            got = plan(n, wb, host, avail)
            assert 0 < got <= avail, (n, wb, host, got, avail)
            full = plan(n, wb, host, 1 << 62)
            reduced = plan(n, wb, host, 0)
            assert got == (full if full <= avail else reduced), (n, wb, host)
            # the reduced layout is the full one without X / Xs: (n + 2) list entries of 8 + wb bytes, aligned
            if n < (1 << 32):
                assert 0 < full - reduced - (n + 2) * (8 + wb) < 1024, (n, wb, host)
            else:
                assert full == reduced
            assert plan(n, wb, 0, 1 << 62) == backend_lib.dq_sufsort_hip_workspace_bytes(n, wb)
            assert plan(n, wb, 1, 1 << 62) - plan(n, wb, 0, 1 << 62) >= wb * n        # the host entry's SAbuf
    # just below 2^32 only the reduced layout fits; it is chosen there, and the full one where it fits
    n = (1 << 32) - 1
    assert plan(n, 8, 1, 1 << 62) > HBM >= plan(n, 8, 1, HBM)
    assert plan(3 << 30, 8, 1, HBM) == plan(3 << 30, 8, 1, 1 << 62)
    assert plan((1 << 32) + 1, 8, 1, HBM) == -1
    assert plan(1 << 31, 4, 1, HBM) == -1
    assert plan(1 << 20, 3, 1, HBM) == -1
    assert plan(-1, 8, 1, HBM) == -1


def test_argument_validation_precedes_device_use(backend_lib):
    from deltaq_amd import _abi
    buf = np.zeros(8, np.uint8)
    sa = np.zeros(8, np.int32)
    assert backend_lib.dq_sufsort_hip_i32(buf.ctypes.data, -1, sa.ctypes.data, 0) == _abi.DQ_ERR_BAD_ARGS
    assert backend_lib.dq_sufsort_hip_i32(None, 8, sa.ctypes.data, 0) == _abi.DQ_ERR_BAD_ARGS
    assert backend_lib.dq_sufsort_hip_i32(buf.ctypes.data, 8, None, 0) == _abi.DQ_ERR_BAD_ARGS
    assert backend_lib.dq_sufsort_hip_i32(buf.ctypes.data, 1 << 31, sa.ctypes.data, 0) == _abi.DQ_ERR_TOO_LARGE
    assert b"2^31" in backend_lib.dq_last_error()
    # the 64-bit entry points take n <= 2^32: one byte more is refused before the device is even looked for
    sa8 = np.zeros(8, np.int64)
    for fn in (lambda: backend_lib.dq_sufsort_hip_i64(buf.ctypes.data, (1 << 32) + 1, sa8.ctypes.data, 0),
               lambda: backend_lib.dq_sufsort_hip_dev_i64(buf.ctypes.data, (1 << 32) + 1, sa8.ctypes.data, 0, None)):
        assert fn() == _abi.DQ_ERR_TOO_LARGE
        assert b"2^32" in backend_lib.dq_last_error()
    assert backend_lib.dq_sufsort_hip_batch_i32(-1, None, None, None, 1, None) == _abi.DQ_ERR_BAD_ARGS
    assert backend_lib.dq_sufsort_hip_batch_i32(0, None, None, None, 1, None) == _abi.DQ_OK


def test_no_cpu_fallback_without_a_device(backend_lib):
    """On a machine without a GPU the product must fail loudly, never compute on the CPU."""
    from deltaq_amd import HipSuffixSort, SuffixSortError, _abi
    if backend_lib.dq_device_count() > 0:
        pytest.skip("a GPU is present")
    with pytest.raises(SuffixSortError) as ei:
        HipSuffixSort().Sort(b"banana")
    assert ei.value.code == _abi.DQ_ERR_NO_DEVICE


def test_missing_library_fails_loudly(monkeypatch, tmp_path):
    from deltaq_amd import _abi
    monkeypatch.setattr(_abi, "_lib", None)
    monkeypatch.setenv("DQ_SUFSORT_LIB", str(tmp_path / "nope.so"))
    with pytest.raises(_abi.BackendMissingError):
        _abi.load()


def test_length_mismatch_matches_reference_message(backend_lib):
    # LibDivSufSort.cs:23-31: ArgumentException("Text and suffix buffers should have the same length")
    from deltaq_amd import HipSuffixSort
    with pytest.raises(ValueError, match="Text and suffix buffers should have the same length"):
        HipSuffixSort().Sort(b"abcdef", np.zeros(5, np.int32))
    with pytest.raises(TypeError):
        HipSuffixSort().Sort(b"abcdef", np.zeros(6, np.float32))


def test_product_never_imports_the_oracle():
    """oracle/ is test infrastructure: nothing under deltaq_amd/ may reference it."""
    pkg = os.path.join(ROOT, "deltaq_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".h", ".hip", ".cpp")):
                src = open(os.path.join(dirpath, f), errors="replace").read()
                assert "import oracle" not in src and "from oracle" not in src, f
                assert "dq_oracle" not in src, f


# ---- the never-compiled C# shim (no dotnet in any image): its [DllImport] signatures against the header
C_WIDTH = {"int32_t": "i32", "int64_t": "i64", "void": "void", "double": "f64"}
CS_WIDTH = {"int": "i32", "long": "i64", "void": "void", "double": "f64", "uint": "i32", "ulong": "i64"}


def c_kind(decl: str) -> str:
    """'i32' / 'i64' for integers by value, 'ptr' for any pointer, 'void'."""
    decl = decl.replace("const", " ").strip()
    if "*" in decl:
        return "ptr"
    base = decl.split()[0]
    assert base in C_WIDTH, decl
    return C_WIDTH[base]


def cs_kind(decl: str) -> str:
    decl = decl.strip()
    if "*" in decl or decl.split()[0] in ("IntPtr", "UIntPtr") or decl.startswith(("ref ", "out ")):
        return "ptr"
    base = decl.split()[0]
    assert base in CS_WIDTH, decl
    return CS_WIDTH[base]


def header_signatures():
    text = open(os.path.join(ROOT, "include", "dq_sufsort.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    sigs = {}
    for ret, name, args in re.findall(r"^\s*([A-Za-z_][\w \*]*?)\s*\b(dq_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text, flags=re.M):
        params = [] if args.strip() in ("", "void") else [c_kind(a) for a in args.split(",")]
        sigs[name] = (c_kind(ret), params)
    return sigs


def csharp_signatures():
    sigs = {}
    base = os.path.join(ROOT, "bindings", "csharp")
    for dirpath, _, files in os.walk(base):
        for f in files:
            if not f.endswith(".cs"):
                continue
            text = re.sub(r"//[^\n]*", "", open(os.path.join(dirpath, f)).read())
            for attrs, ret, name, args in re.findall(
                    r"\[DllImport\(([^\]]*)\)\]\s*(?:(?:internal|private|public|static|extern|unsafe)\s+)+([\w\*]+)\s+(dq_\w+)\s*\(([^)]*)\)\s*;",
                    text, flags=re.S):
                assert "CallingConvention.Cdecl" in attrs, f"{f}: {name} must be Cdecl"
                assert "EntryPoint" not in attrs, f"{f}: {name} renames its entry point"
                params = [] if not args.strip() else [cs_kind(a) for a in args.split(",")]
                sigs.setdefault(name, []).append((f, cs_kind(ret), params))
    return sigs


def test_csharp_dllimports_match_the_header():
    """Every [DllImport] of bindings/csharp/**/*.cs names an export of include/dq_sufsort.h with the same arity, the same
    integer widths by value (C# int = int32_t, long = int64_t) and pointers where the header has pointers."""
    hdr, cs = header_signatures(), csharp_signatures()
    assert len(hdr) == len(header_symbols())            # the signature parser sees every declaration
    assert cs, "no [DllImport] found under bindings/csharp"
    assert {"dq_sufsort_hip_i32", "dq_bsdiff_create", "dq_bspatch_apply", "dq_bsdiff_search_i32", "dq_bsdiff_index_create",
            "dq_bsdiff_index_diff", "dq_bsdiff_index_free"} <= set(cs)
    for name, uses in cs.items():
        assert name in hdr, f"{name}: imported by {uses[0][0]} but not declared in include/dq_sufsort.h"
        ret, params = hdr[name]
        for f, cret, cparams in uses:
            # `const char *` comes back as IntPtr
            assert cret == ret, f"{f}: {name} returns {cret}, header says {ret}"
            assert len(cparams) == len(params), f"{f}: {name} takes {len(cparams)} arguments, header says {len(params)}"
            assert cparams == params, f"{f}: {name} argument kinds {cparams} differ from the header's {params}"


# ---- the dq_last_*_info records: dq_call_info.h's structs against _abi.py's table, and the getters' edges
def header_records():
    """{export name: [field names, in order]} parsed out of deltaq_amd/csrc/dq_call_info.h: struct <Name>Info is the record
    behind dq_last_<name>_info."""
    text = open(os.path.join(ROOT, "deltaq_amd", "csrc", "dq_call_info.h")).read()
    text = re.sub(r"//[^\n]*", "", text)
    records = {}
    for name, body in re.findall(r"\bstruct\s+(\w+Info)\s*\{(.*?)\};", text, flags=re.S):
        fields = []
        for decl in body.split(";"):
            if decl.strip():
                m = re.fullmatch(r"\s*int64_t\s+([\w\s,]+)", decl)
                assert m, f"{name}: a member that is no int64_t field: {decl.strip()!r}"
                fields += [f.strip() for f in m.group(1).split(",")]
        records["dq_last_" + re.sub(r"(?<!^)(?=[A-Z])", "_", name).lower()] = fields
        assert re.search(rf"static_assert\(sizeof\({name}\) == {len(fields)} \* sizeof\(int64_t\)\)", text), name
    return records


def test_python_record_table_matches_the_header_structs():
    """One name per counter: _abi.RECORDS has the records of dq_call_info.h, each with as many fields in the same order,
    and every Python key is the field's name -- ..._ms for ..._us exactly where the scale is 1e-3."""
    from deltaq_amd import _abi
    hdr = header_records()
    assert len(hdr) == 9 and set(hdr) == set(_abi.RECORDS)
    assert set(hdr) <= set(header_symbols())
    for export, fields in hdr.items():
        table = _abi.RECORDS[export]
        assert len(table) == len(fields) == len(set(fields)), export
        for field, (key, scale) in zip(fields, table):
            assert scale in (1, 1e-3), (export, key)
            if scale == 1e-3:
                assert field.endswith("_us") and key == field[:-3] + "_ms", (export, field, key)
            else:
                assert key == field and not field.endswith("_us"), (export, field, key)


def test_info_getters_zero_fill_and_reject_bad_arguments(backend_lib):
    """The eight array getters on a fresh thread (no GPU use: its records are all zero): count = fields + 3 fills every
    slot, the extra ones with zeros; count = 0 succeeds and writes nothing; a NULL array and a negative count are
    DQ_ERR_BAD_ARGS."""
    import threading
    from deltaq_amd import _abi
    getters = [name for name in _abi.RECORDS if name != "dq_last_sort_info"]
    assert len(getters) == 8
    failures = []

    def work():
        try:
            for name in getters:
                fn, n = getattr(backend_lib, name), len(_abi.RECORDS[name])
                v = (ctypes.c_int64 * (n + 3))(*([-7] * (n + 3)))
                assert fn(v, n + 3) == _abi.DQ_OK and list(v) == [0] * (n + 3), (name, list(v))
                v = (ctypes.c_int64 * 1)(-7)
                assert fn(v, 0) == _abi.DQ_OK and v[0] == -7, name
                assert fn(None, n) == _abi.DQ_ERR_BAD_ARGS and backend_lib.dq_last_error(), name
                assert fn(v, -1) == _abi.DQ_ERR_BAD_ARGS and v[0] == -7, name
        except Exception as e:                                          # noqa: BLE001 -- reported below
            failures.append(e)

    t = threading.Thread(target=work)
    t.start()
    t.join()
    assert not failures, failures
