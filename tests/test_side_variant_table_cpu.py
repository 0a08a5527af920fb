"""The case table of tests/side_variant_table.py against the built side libraries: for every name in the Makefile's SIDE, every kernel
in the gfx950 code objects of libqle_<name>.so has a row, every row names a kernel its library has, no two kernels demangle to one id,
and every kernel has an exported host handle (the symbol the library's launch census names it by).  The SIDE list is read from the
Makefile, so a library without rows fails here.  No count is written down: the lists are read from the libraries.  Every row's inputs
are held to the conditions that keep it from hiding a failure (side_variant_table.conditions), on the reference alone."""
import os
import re

import pytest

import side_variant_table as st
from elf_util import _gfx950_code_objects, _kernels, _symbols
from quadrotor_landing_amd import _lib
from side_lib_util import CSRC, ensure_built


def makefile_side():
    m = re.search(r"^SIDE\s*:=\s*(.+)$", open(os.path.join(CSRC, "Makefile")).read(), flags=re.M)
    assert m, "csrc/Makefile has no SIDE list"
    return m.group(1).split()


SIDE = makefile_side()


@pytest.fixture(scope="module", params=SIDE)
def library(request):
    name = request.param
    path = ensure_built(name)
    d = open(path, "rb").read()
    return dict(name=name, units=len(_gfx950_code_objects(d)), mangled=_kernels(path), dynsym=set(_symbols(d, 11)))


def test_the_makefile_list_and_the_package_agree():
    assert len(SIDE) == len(set(SIDE)) and SIDE
    assert set(SIDE) == set(_lib.SIDE_LIBRARIES), sorted(set(SIDE) ^ set(_lib.SIDE_LIBRARIES))
    no_rows = [n for n in SIDE if not st.rows_of(n)]
    assert not no_rows, f"side libraries without a row in tests/side_variant_table.py: {no_rows}"
    assert {r["library"] for r in st.ROWS} <= set(SIDE)
    assert {lib for r in st.ROWS for lib, _ in r["kernels"]} <= set(SIDE)
    assert st.EXCLUDED == {}


def test_every_kernel_has_a_row_and_every_row_a_kernel(library):
    name = library["name"]
    assert library["units"] > 0 and library["mangled"], f"no gfx950 kernel descriptor found in libqle_{name}.so"
    ids = {st.kernel_id(_lib.demangle(m)) for m in library["mangled"]}
    assert len(ids) == len(library["mangled"]), "two kernels demangle to one id"
    rows = st.covered_kernels(name)
    no_row = sorted(ids - rows - {k for lib, k in st.EXCLUDED if lib == name})
    assert not no_row, f"{len(no_row)} kernel(s) of libqle_{name}.so have no row in tests/side_variant_table.py: " + "; ".join(no_row[:20])
    missing = sorted(rows - ids)
    assert not missing, f"{len(missing)} row kernel(s) are not in libqle_{name}.so: " + "; ".join(missing[:20])
    # the kernels of the library's own ladder are launched by rows of that library (the pack of devio rides along in others' rows)
    own = set().union(*({k for lib, k in r["kernels"] if lib == name} for r in st.rows_of(name)))
    assert own == ids, sorted(ids - own)[:20]


def test_every_kernel_has_an_exported_host_handle(library):
    """The census names a launch by the dynamic symbol of the kernel's host handle (side_host.hpp: dladdr first): it must exist for
    every device kernel, and every host handle of a kernel family must have a device kernel."""
    missing = sorted(library["mangled"] - library["dynsym"])
    assert not missing, f"kernels without an exported host handle: {[_lib.demangle(m) for m in missing[:10]]}"
    families = {k.split("<")[0] for k in st.covered_kernels(library["name"])}
    handles = {s for s in library["dynsym"] if s.startswith("_Z") and st.kernel_id(_lib.demangle(s)).split("<")[0] in families}
    assert handles <= library["mangled"], sorted(handles - library["mangled"])[:10]


def test_rows_are_well_formed():
    for r in st.ROWS:
        assert r["kernels"] and r["reference"] and r["record"] in st.RECORDS and r["dtype"] in st.DTYPES, r["id"]
        assert any(lib == r["library"] for lib, _ in r["kernels"]), r["id"]
        assert all(k.startswith("k_") for _, k in r["kernels"]), r["id"]
        if r.get("M") is not None:
            assert (r["M"] * r["G"]) % 64 != 0 or r["M"] == 64, r["id"]     # ragged, or a bank per tile
    assert st.B % 64 != 0 and st.B > 128 and st.SRC_B % 64 != 0 and st.SEQ_K > 32
    assert set(st.ROW_TOL) <= {r["id"] for r in st.ROWS}


@pytest.mark.parametrize("row", st.ROWS, ids=[r["id"] for r in st.ROWS])
def test_the_reference_alone_satisfies_the_rows_conditions(row):
    d = st.conditions(row)
    assert d.B == (st.B if row.get("M") is None else row["M"] * row["G"])
    if row.get("M") is None:
        assert d.mask[:64].all() and 0 < d.mask[64:].sum() < d.B - 64         # one whole tile on, mixed bits elsewhere
        assert not d.x[d.ZERO].any() and not d.P[d.ZERO].any()               # the uninitialised record


def test_kernel_id():
    d = _lib.demangle("_ZN3qsi9k_si_packIfdLi9ELb0EEEvPKT0_S3_PKhPT_l")
    assert st.kernel_id(d) == "k_si_pack<float, double, 9, false>", d


def test_the_census_of_side_host_under_the_sanitizers(tmp_path_factory):
    """tests/cpp/side_census_harness.cpp: the census of csrc/side_host.hpp (the record launch() makes, begin, and end's two-call size
    protocol) in a stand-alone host program, eight threads recording; once as it is and once under AddressSanitizer and UBSan.  No GPU
    call is made.  By clang++, as the stateio harness: the layout header under side_host.hpp declares vector types a host g++ lacks."""
    import subprocess

    import host_harness
    exes = host_harness.build("side_census_harness", tmp_path_factory, cxx="/opt/rocm/lib/llvm/bin/clang++",
                              flags=host_harness.FLAGS[:5] + ("-Wno-unused-variable", "-Wno-pass-failed"),
                              extra=("-rdynamic", "-pthread", "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath,/opt/rocm/lib"))
    for exe in exes:
        r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and r.stdout == "OK\n" and r.stderr == "", (exe, r.returncode, r.stdout, r.stderr[-3000:])
