"""The Python side of the host harnesses under tests/cpp: one place that compiles them (plain, and as stand-alone programs under
AddressSanitizer and UBSan that are run directly), one that writes an input file, runs a program and reads its result, and the
parameter words the harnesses' decode_params reads."""
import os
import subprocess

import numpy as np

CPP = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cpp")
# the product headers compiled by g++: the HIP headers define the device decorators away
FLAGS = ("-I/opt/rocm/include", "-D__HIP_PLATFORM_AMD__", "-Wall", "-Wno-unknown-pragmas", "-Wno-unused-function", "-Wno-maybe-uninitialized",
         "-Wno-unused-but-set-variable")
SANITIZE = ("-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")   # a report ends the program with a non-zero status


def build(name, tmp_path_factory, *, plain=True, sanitized=True, cxx="g++", flags=FLAGS, extra=()):
    """tests/cpp/NAME.cpp compiled into a fresh directory: -> (plain, san), or the one that was asked for alone."""
    d = tmp_path_factory.mktemp(name)
    src, out = os.path.join(CPP, name + ".cpp"), []
    for wanted, suffix, opt in ((plain, "", ("-O2",)), (sanitized, "_san", SANITIZE)):
        if wanted:
            out.append(str(d / (name + suffix)))
            subprocess.run([cxx, "-std=c++17", *opt, *flags, *extra, "-o", out[-1], src], check=True)
    return tuple(out)


def run(exe, tmp, header, payload_arrays, out_shape, argv=()):
    """Write header and payload as doubles to tmp/in.bin, run `exe *argv in.bin out.bin` (harness_main of tests/cpp/harness_io.hpp),
    hold it to status 0, a silent stderr and the batch header[0] on stdout, and return the doubles of out.bin in out_shape."""
    fin, fout = str(tmp / "in.bin"), str(tmp / "out.bin")
    with open(fin, "wb") as fh:
        for a in (header, *payload_arrays):
            np.ascontiguousarray(a, np.float64).tofile(fh)
    r = subprocess.run([exe, *argv, fin, fout], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "" and int(r.stdout) == int(header[0]), (r.returncode, r.stdout, r.stderr[-3000:])
    return np.fromfile(fout, np.float64).reshape(out_shape)


def params_header(po):
    """The 47 doubles of the oracle's parameters `po`, in the order decode_params of tests/cpp/harness_io.hpp reads them."""
    return [po.dT_nom, po.dT_nom if po.est_bias else 0.0, float(po.est_bias), po.small_ang_tol,
            *po.g, *po.q_vc, *po.C_vc, *po.r_v_cv, *po.Q, *po.R, *po.ab_static, *po.wb_static]


def full_P(P, compact=False):
    """[B, n, n] in the corner of [B, 225]: zeros around it, or for a compact record NaN -- those words do not exist."""
    B, n = P.shape[:2]
    P15 = np.full((B, 15, 15), np.nan if compact else 0.0)
    P15[:, :n, :n] = P
    return P15.reshape(B, 225)
