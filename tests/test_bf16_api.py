"""The opt-in bf16 inference path is part of the two public interfaces (no GPU needed): libbcnn.so exports the precision
switch of include/bcnn/bcnn.h, libbcnn_hip.so the operator of include/bcnn_hip.h, both headers declare them, and the
Python bindings know them."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "bcnn_amd", "lib")


def _exports(lib):
    r = subprocess.run(["nm", "-D", "--defined-only", os.path.join(LIB, lib)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return {line.split()[-1] for line in r.stdout.splitlines() if " T " in line}


def _header(*path):
    return re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", *path)).read(), flags=re.S)


def test_libbcnn_exports_the_precision_switch():
    syms = _exports("libbcnn.so")
    assert {"bcnn_set_inference_precision", "bcnn_get_inference_precision"} <= syms


def test_libbcnn_hip_exports_the_operator():
    assert "bcnn_hip_conv_forward_bf16" in _exports("libbcnn_hip.so")


def test_the_headers_declare_them():
    pub = _header("bcnn", "bcnn.h")
    assert re.search(r"BCNN_API\s+bcnn_status\s+bcnn_set_inference_precision\s*\(\s*bcnn_net\s*\*\s*\w+\s*,\s*bcnn_precision\s+\w+\s*\)\s*;", pub)
    assert re.search(r"BCNN_API\s+bcnn_precision\s+bcnn_get_inference_precision\s*\(\s*const\s+bcnn_net\s*\*\s*\w+\s*\)\s*;", pub)
    assert re.search(r"BCNN_PRECISION_FP32\s*=\s*0\s*,\s*BCNN_PRECISION_BF16\s*=\s*1\s*}\s*bcnn_precision\s*;", pub)
    hip = _header("bcnn_hip.h")
    m = re.search(r"\bint\s+bcnn_hip_conv_forward_bf16\s*\(([^)]*)\)\s*;", hip)
    assert m
    fwd = re.search(r"\bvoid\s+bcnn_hip_conv_forward\s*\(([^)]*)\)\s*;", hip)
    norm = lambda s: re.sub(r"\s+", " ", s).strip()
    assert norm(m.group(1)) == norm(fwd.group(1)), "the bf16 operator takes the argument list of bcnn_hip_conv_forward"


def test_the_python_bindings_know_them():
    from bcnn_amd import _lib, capi, ops
    assert "bcnn_hip_conv_forward_bf16" in _lib.declared_symbols() and "bcnn_hip_conv_forward_bf16" in _lib.SIGNATURES
    assert _lib.SIGNATURES["bcnn_hip_conv_forward_bf16"][1] == _lib.SIGNATURES["bcnn_hip_conv_forward"][1]
    assert callable(ops.conv_forward_bf16) and callable(capi.Net.set_inference_precision)
    assert (capi.PRECISION_FP32, capi.PRECISION_BF16) == (0, 1)
