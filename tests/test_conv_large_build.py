"""What of the large-kernel convolution family (bcnn_amd/csrc/conv_large.hip) can be checked without a
GPU: its kernels, and the split-K finalize and per-tap reduce kernels of conv_bwd.hip (the family's weight gradient ends in
the former), compile for gfx950 without scratch memory (a spilled accumulator or staging register turns the
inner loop into scratch traffic that nothing but the code object shows), the family is wired into the three dispatch
ladders ahead of the catch-all kernels. With a GPU: an INI graph with an 11x11 / s4 layer loads through bcnn_load_net (the
loader allocates device tensors, so that one test carries the gpu marker)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "bcnn_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

ALEXNET_STEM_CFG = """
[network]
input_width=67
input_height=67
input_channels=3
batch_size=2
optimizer=sgd
learning_rate=0.01

[convolutional]
filters=96
size=11
stride=4
pad=0
function=relu
src=input
dst=conv1

[maxpool]
size=3
stride=2
src=conv1
dst=pool1

[convolutional]
filters=32
size=9
stride=1
pad=4
bn=1
function=relu
src=pool1
dst=conv2

[connected]
output=10
src=conv2
dst=fc

[softmax]
src=fc
dst=sm

[cost]
src=sm
dst=cost
"""


@pytest.fixture(scope="module")
def metadata(tmp_path_factory):
    """kernel name -> bytes of scratch per work-item, from the code object metadata of the compiled files: the family's own,
    and conv_bwd.hip, which holds the finalize kernel the family shares (and the per-tap reduce kernel next to it)"""
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not found")
    found = {}
    for source in ("conv_large.hip", "conv_bwd.hip"):
        out = tmp_path_factory.mktemp("isa") / (source[:-4] + ".s")
        cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-Wno-unused-function",
               "-Wno-inline-asm", "-S", "--cuda-device-only", "-o", str(out), source]
        r = subprocess.run(cmd, cwd=SRC, capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stderr[-2000:]
        for name, size in re.findall(r"\.name:\s+(\S+)\s*\n\s*\.private_segment_fixed_size:\s+(\d+)", out.read_text()):
            assert name not in found, name
            found[name] = int(size)
    return found


@pytest.mark.parametrize("kernel,instances", [("conv_large_gemm_kernel", 4), ("conv_large_dw_kernel", 3),
                                              ("conv_dw_finalize_kernel", 2), ("conv_dw_taps_reduce_kernel", 1)])
def test_kernels_use_no_scratch(metadata, kernel, instances):
    mine = {k: v for k, v in metadata.items() if kernel in k}
    assert len(mine) == instances, (kernel, sorted(metadata))
    for name, scratch in mine.items():
        assert scratch == 0, "%s spills: %d bytes of scratch per work-item" % (name, scratch)


def test_the_family_sits_in_front_of_the_catch_all_kernels():
    text = open(os.path.join(SRC, "conv.hip")).read()
    for table, large, behind in (("kConvFwdFamilies", "conv_forward_large", ("conv_forward_dma_timed", "conv_forward_small_c",
                                                                             "conv_forward_igemm")),
                                 ("kConvDxFamilies", "conv_backward_data_large", ("conv_backward_data_small_c",
                                                                                  "conv_backward_data_dma", "conv_backward_data_igemm"))):
        rows = re.search(table + r"\[\]\s*=\s*\{(.*?)\n\};", text, re.S).group(1)
        for name in behind:
            assert rows.index(large) < rows.index(name), (table, name)
    rows = re.search(r"kDwFamilies\[\]\s*=\s*\{(.*?)\n\};", text, re.S).group(1)
    assert rows.index("conv_backward_weights_large") < rows.index("{conv_dw_workspace_floats")
    assert "conv_large.hip" in open(os.path.join(SRC, "Makefile")).read()


@pytest.mark.gpu  # bcnn_load_net allocates the tensors it declares on the device
def test_an_ini_graph_with_an_11x11_stride_4_layer_loads(tmp_path):
    from bcnn_amd import capi
    cfg = tmp_path / "alexnet_stem.cfg"
    cfg.write_text(ALEXNET_STEM_CFG)
    net = capi.Net.load_net(str(cfg), None, capi.MODE_TRAIN)
    assert net.num_nodes == 6
    c1, c2 = net.index("conv1"), net.index("conv2")
    assert net.shape(c1) == (2, 96, 15, 15) and net.shape(c2) == (2, 32, 8, 8)
    wshape = net.shape(net.index("input_w"))  # a conv node names its weights after its source
    assert int(wshape[0] * wshape[1] * wshape[2] * wshape[3]) == 96 * 3 * 11 * 11
    net.close()
