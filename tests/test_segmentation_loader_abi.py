"""CPU checks of the segmentation-list loader's entry points: the public headers declare the new
names once each, the loader constant sits behind the enumerator list (BCNN_NUM_LOADERS + 1), the libraries export the
symbols, bcnn_amd._lib / ops / capi expose the names, bcnn_set_data_loader refuses the new type on a net without a
softmax-loss node and leaves no loader behind, and tools/label_warp_check.c passes under the host sanitizers as a
stand-alone program. Every loader test that builds a net is in tests/test_segmentation_loader.py (gpu)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

from tests.test_data_loader import _write_cifar

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _no_comments(text):
    return re.sub(r"/\*.*?\*/|//[^\n]*", "", text, flags=re.S)


def _header(*parts):
    return _no_comments(open(os.path.join(ROOT, "include", *parts)).read())


def test_headers_declare_the_names_once_each():
    public = _header("bcnn", "bcnn.h")
    value = re.findall(r"#define\s+BCNN_LOAD_SEGMENTATION_LIST\s+(.*)", public)
    assert len(value) == 1
    assert re.sub(r"\s+", "", value[0]) == "((bcnn_loader_type)(BCNN_NUM_LOADERS+1))"
    # the enumerator list is untouched: it still ends BCNN_LOAD_DETECTION_LIST, BCNN_NUM_LOADERS (= 5, the reference's)
    body = re.search(r"typedef\s+enum\s*\{([^}]*)\}\s*bcnn_loader_type\s*;", public).group(1)
    names = [t.strip() for t in body.split(",") if t.strip()]
    assert names[-2:] == ["BCNN_LOAD_DETECTION_LIST", "BCNN_NUM_LOADERS"] and len(names) == 6
    assert len(re.findall(r"BCNN_API\s+int\s+bcnn_get_loader_device_labels\s*\(\s*const\s+bcnn_net\s*\*\s*net\s*\)\s*;", public)) == 1
    hip = _header("bcnn_hip.h")
    decl = re.findall(r"\bint\s+bcnn_hip_augment_label_batch\s*\(([^;{]*)\)\s*;", hip)
    assert len(decl) == 1
    assert re.sub(r"\s+", " ", decl[0]).strip() == (
        "float *label_d, int n, int h, int w, int num_samples, const uint8_t *maps, "
        "const bcnn_hip_augment_record *records, const int32_t *taps, int fill")
    bip = _header("bip", "bip.h")
    for name in ("bip_load_index_map", "bip_load_index_map_from_memory", "bip_warp_label_map"):
        assert len(re.findall(r"\bbip_status\s+%s\s*\([^;{]*\)\s*;" % name, bip)) == 1, name


def test_libraries_export_the_symbols():
    from bcnn_amd import _lib, capi
    assert hasattr(C.CDLL(_lib.LIB_PATH), "bcnn_hip_augment_label_batch")
    assert "bcnn_hip_augment_label_batch" in _lib.SIGNATURES and "bcnn_hip_augment_label_batch" in _lib.declared_symbols()
    assert len(_lib.SIGNATURES["bcnn_hip_augment_label_batch"][1]) == 9
    host = C.CDLL(capi.LIB_PATH)
    assert hasattr(host, "bcnn_get_loader_device_labels") and hasattr(host, "bcnn_loader_fill_record")
    bip = C.CDLL(os.path.join(os.path.dirname(capi.LIB_PATH), "libbip.so"))
    for name in ("bip_load_index_map", "bip_load_index_map_from_memory", "bip_warp_label_map"):
        assert hasattr(bip, name), name


def test_python_names():
    from bcnn_amd import capi, ops
    assert callable(ops.augment_label_batch) and callable(ops.warp_label_map)
    assert capi.LOAD_SEGMENTATION_LIST == 6 and capi.LOAD_DETECTION_LIST == 4
    for name in ("set_data_loader", "loader_next", "loader_device_labels"):
        assert callable(getattr(capi.Net, name)), name


def _open_paths():
    return {os.path.realpath(os.path.join("/proc/self/fd", f)) for f in os.listdir("/proc/self/fd")
            if os.path.exists(os.path.join("/proc/self/fd", f))}


def test_the_new_type_is_refused_without_a_softmax_loss_node_and_leaves_no_loader(tmp_path, capfd):
    from bcnn_amd import capi
    L = capi.lib()
    net = C.c_void_p()
    assert L.bcnn_init_net(C.byref(net), capi.MODE_TRAIN) == 0   # host allocations only
    # the net is not ended: bcnn_end_net synchronises the device, and this test runs without one
    L.bcnn_set_log_context(net, None, 2)                          # BCNN_LOG_ERROR: the refusal goes to stderr
    L.bcnn_set_input_shape(net, 32, 32, 3, 2)
    assert L.bcnn_get_loader_device_labels(net) == 0 and L.bcnn_get_loader_device_labels(None) == 0
    cifar = _write_cifar(tmp_path, "data_batch_1", 3)
    lst = tmp_path / "seg.txt"
    lst.write_text("a.png a_mask.png\n")
    for kind in (7, 5, -1, 99):                                   # BCNN_NUM_LOADERS itself names no loader, nor does 7
        assert L.bcnn_set_data_loader(net, kind, str(lst).encode(), None, None, None) == 1
    # a CIFAR loader (host buffers and one open file) is in place ...
    assert L.bcnn_set_data_loader(net, capi.LOAD_CIFAR10, cifar.encode(), None, None, None) == 0
    assert os.path.realpath(cifar) in _open_paths()
    capfd.readouterr()
    # ... the segmentation list is refused, with its reason, before it opens anything ...
    assert L.bcnn_set_data_loader(net, capi.LOAD_SEGMENTATION_LIST, str(lst).encode(), None, None, None) == 1   # BCNN_INVALID_PARAMETER
    assert "softmax-loss" in capfd.readouterr().err
    # ... and no loader is left: the old one is closed and the list was never opened
    opened = _open_paths()
    assert os.path.realpath(cifar) not in opened and os.path.realpath(str(lst)) not in opened


def test_label_warp_check_passes_under_the_host_sanitizers(tmp_path):
    """tools/label_warp_check.c with its own main, compiled with -fsanitize=address,undefined and run as a program: the
    rule over heap maps of exactly w * h bytes. Skipped only where cc cannot link the sanitizer runtimes."""
    cc = shutil.which("cc") or shutil.which("gcc")
    if cc is None:
        pytest.skip("no C compiler")
    probe = tmp_path / "probe.c"
    probe.write_text("int main(void) { return 0; }\n")
    flags = ["-std=gnu99", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    if subprocess.run([cc] + flags + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("cc lacks the sanitizer runtime")
    exe = str(tmp_path / "label_warp_check")
    subprocess.run([cc] + flags + [os.path.join(ROOT, "tools", "label_warp_check.c"), "-lm", "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and run.stdout.strip() == "ok", (run.returncode, run.stdout, run.stderr[-2000:])
