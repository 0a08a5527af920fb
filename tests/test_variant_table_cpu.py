"""The case table of tests/variant_table.py against the built library: every kernel in the gfx950 code objects of libqle_ekf.so has a
row (or is a listed helper), every row names a kernel the library has, and every kernel has an exported host handle (the symbol the
launch census names it by).  No count is written down: the lists are read from the library."""
import os

import pytest

import variant_table as vt
from elf_util import _gfx950_code_objects, _kernels, _symbols
from quadrotor_landing_amd import _lib


@pytest.fixture(scope="module")
def library():
    d = open(_lib.LIB_PATH, "rb").read()
    return dict(units=len(_gfx950_code_objects(d)), mangled=_kernels(_lib.LIB_PATH), dynsym=set(_symbols(d, 11)))


def test_every_kernel_has_a_row_and_every_row_a_kernel(library):
    assert library["units"] > 0 and library["mangled"], "no gfx950 kernel descriptor found in libqle_ekf.so"
    ids = {vt.kernel_id(_lib.demangle(m)) for m in library["mangled"]}
    assert len(ids) == len(library["mangled"]), "two kernels demangle to one id"
    helpers = {k for k in ids if k.split("<")[0] in vt.HELPER_FAMILIES}
    rows = vt.covered_kernels()
    no_row = sorted(ids - rows - helpers - set(vt.EXCLUDED))
    assert not no_row, f"{len(no_row)} kernel(s) of the library have no row in tests/variant_table.py: " + "; ".join(no_row[:20])
    missing = sorted(rows - ids)
    assert not missing, f"{len(missing)} row kernel(s) are not in the library: " + "; ".join(missing[:20])
    assert not set(vt.EXCLUDED) - ids, "EXCLUDED names kernels the library lacks"
    unknown_helper = sorted(f for f in vt.HELPER_FAMILIES if not any(k.split("<")[0] == f for k in helpers))
    assert not unknown_helper, f"helper families without a kernel: {unknown_helper}"


def test_every_kernel_has_an_exported_host_handle(library):
    """The census names a launch by the dynamic symbol of the kernel's host handle: it must exist for every device kernel, and
    every host handle of the library must have a device kernel."""
    missing = sorted(library["mangled"] - library["dynsym"])
    assert not missing, f"kernels without an exported host handle: {[_lib.demangle(m) for m in missing[:10]]}"
    handles = {s for s in library["dynsym"] if vt.kernel_id(_lib.demangle(s)).split("<")[0] in
               {k.split("<")[0] for k in vt.covered_kernels()} | set(vt.HELPER_FAMILIES)}
    assert handles <= library["mangled"], sorted(handles - library["mangled"])[:10]


def test_rows_are_well_formed():
    groups = vt.groups()
    for key, rows in groups.items():
        assert rows[0]["canonical"]
        assert len({r["dtype"] for r in rows}) == 1 and len({r["entry"] for r in rows}) == 1
        for r in rows:
            assert r["kernels"], r["id"]
            assert all(k.startswith(("k_", "kw_")) for k in r["kernels"])
            assert set(r["env"]) <= {"QLE_COMPACT", "QLE_NT", "QLE_REFRESH", "QLE_SPLIT", "QLE_LOADS_FIRST", "QLE_QUAD", "QLE_BLOCK"}
            # a row's batch gives at least 8 workgroups at its block size, and not a multiple of 8
            blk = int(r["env"].get("QLE_BLOCK", 64))
            wg = -(-r["B"] // blk) if not r["entry"].startswith("kw_") else -(-r["B"] // 64) * (4 if r["B"] <= 4096 else 1)
            assert wg >= 8 and wg % 8 != 0 and r["B"] % 64 != 0, (r["id"], wg)


def test_demangle_and_kernel_id():
    m = "_ZN3qle6k_stepIfLb1ELb0ELb1ELi2ELb0EEEvPT_PKS1_S4_llii"
    d = _lib.demangle(m)
    assert vt.kernel_id(d) == "k_step<float, true, false, true, 2, false>", d
    assert _lib.demangle("not_mangled") == "not_mangled"
    assert os.path.exists(_lib.LIB_PATH)
