"""The inference-precision switch of a net (bcnn_set_inference_precision, include/bcnn/bcnn.h) through
capi.Net, on a small graph: conv 3->8 3x3 p1 ReLU, maxpool 2, conv 8->16 1x1 ReLU, conv 16->8 3x3 s2 p1; N = 2, 3x16x16.

Inputs and weights come from {-1, 0, 1} and the biases are 0, so every activation is an integer of magnitude
<= 27 * 8 = 216 < 256 (exact in bf16) and every sum is exact in fp32: a bf16 forward has to give the bits of the fp32 one.
The dispatch trace says which kernel families ran."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

BF16_FAMILY = "conv_bf16_gemm_kernel"
# what the fp32 forward families call themselves in the trace (the rows of kConvFwdFamilies, conv.hip)
FP32_FAMILIES = {"conv_fwd_window_kernel", "conv_fwd_stem_kernel", "conv_fwd_direct_kernel", "wino43b_kernel:fwd",
                 "wino_fused_kernel:fwd", "wino_unfused:fwd", "conv_large_gemm_kernel:fwd", "conv_igemm_dma_kernel:fwd",
                 "conv_igemm_kernel:fwd"}
N_CONV = 3


def _trace_start():
    from bcnn_amd import _lib
    _lib.load().bcnn_hip_trace_enable(1)


def _trace_stop():
    """the kernel families named since _trace_start, in launch order"""
    from bcnn_amd import _lib
    L = _lib.load()
    n = L.bcnn_hip_trace_read(None, 0)
    buf = ctypes.create_string_buffer(n + 1)
    L.bcnn_hip_trace_read(buf, n + 1)
    L.bcnn_hip_trace_enable(0)
    return buf.value.decode().split()


def _net(mode, seed=3):
    from bcnn_amd import capi
    net = capi.Net(mode=mode, n=2, w=16, h=16, c=3)
    net.conv(8, 3, 1, 1, 1, 0, capi.ACT_RELU, "input", "c1")
    net.maxpool(2, 2, capi.PADDING_SAME, "c1", "p1")
    net.conv(16, 1, 1, 0, 1, 0, capi.ACT_RELU, "p1", "c2")
    net.conv(8, 3, 2, 1, 1, 0, capi.ACT_NONE, "c2", "c3")
    net.compile()
    rs = np.random.RandomState(seed)
    for name in ("input", "input_w", "p1_w", "c2_w"):   # a conv node names its weights after its source
        i = net.index(name)
        net.data(i)[...] = rs.randint(-1, 2, net.shape(i)).astype(np.float32)
        net.upload(i)
    for name in ("input_b", "p1_b", "c2_b"):
        i = net.index(name)
        net.data(i)[...] = 0.0
        net.upload(i)
    return net


def _forward(net):
    """(output of the last node, trace of the pass)"""
    _trace_start()
    net.forward()
    net.sync()
    names = _trace_stop()
    out = net.index("c3")
    net.download(out, with_grad=False)
    return net.data(out).copy(), names


def test_predict_net_in_bf16_gives_the_bits_of_fp32_and_runs_the_bf16_family():
    from bcnn_amd import capi
    net = _net(capi.MODE_PREDICT)
    assert net.get_inference_precision() == capi.PRECISION_FP32
    y32, names32 = _forward(net)
    assert BF16_FAMILY not in names32
    assert sum(names32.count(k) for k in FP32_FAMILIES) == N_CONV, names32   # every fp32 forward family names itself
    assert float(np.abs(y32).max()) > 0

    assert net.set_inference_precision(capi.PRECISION_BF16) == 0
    assert net.get_inference_precision() == capi.PRECISION_BF16
    y16, names16 = _forward(net)
    assert names16.count(BF16_FAMILY) == N_CONV, names16
    assert not (FP32_FAMILIES & set(names16)), names16
    assert np.array_equal(y16.view(np.uint32), y32.view(np.uint32))

    assert net.set_inference_precision(capi.PRECISION_FP32) == 0
    y32b, names32b = _forward(net)
    assert names32b == names32
    assert np.array_equal(y32b.view(np.uint32), y32.view(np.uint32))
    net.close()


def test_a_train_mode_pass_never_uses_it_and_set_mode_switches_it_on():
    from bcnn_amd import capi
    plain = _net(capi.MODE_TRAIN)
    y_plain, names_plain = _forward(plain)
    plain.close()

    net = _net(capi.MODE_TRAIN)
    assert net.set_inference_precision(capi.PRECISION_BF16) == 0
    y_train, names_train = _forward(net)
    assert BF16_FAMILY not in names_train
    assert names_train == names_plain
    assert np.array_equal(y_train.view(np.uint32), y_plain.view(np.uint32))

    assert net.set_mode(capi.MODE_PREDICT) == 0
    y_pred, names_pred = _forward(net)
    assert names_pred.count(BF16_FAMILY) == N_CONV, names_pred
    assert np.array_equal(y_pred.view(np.uint32), y_plain.view(np.uint32))   # exact data: the same bits again
    net.close()


def test_an_unknown_value_is_refused_and_changes_nothing():
    from bcnn_amd import capi
    net = _net(capi.MODE_PREDICT)
    assert net.set_inference_precision(capi.PRECISION_BF16) == 0
    for bad in (2, -1, 7):
        assert net.set_inference_precision(bad) == 1      # BCNN_INVALID_PARAMETER
        assert net.get_inference_precision() == capi.PRECISION_BF16
    net.close()


@pytest.mark.parametrize("value,want", [("bf16", 1), ("fp32", 0), (None, 0)])
def test_the_loader_reads_inference_precision_from_the_net_section(tmp_path, value, want):
    from bcnn_amd import capi
    cfg = tmp_path / "net.ini"
    cfg.write_text("[net]\ninput_width=16\ninput_height=16\ninput_channels=3\nbatch_size=2\n" +
                   ("inference_precision=%s\n" % value if value else "") +
                   "[conv]\nsrc=input\nfilters=8\nsize=3\nstride=1\npad=1\nfunction=relu\ndst=c1\n")
    net = capi.Net.load_net(str(cfg), mode=capi.MODE_PREDICT)
    assert net.get_inference_precision() == want
    assert net.num_nodes == 1
    if want:
        assert net.L.bcnn_compile_net(net.net) == 0      # bcnn_load_net builds the graph; compiling allocates the input
        net.data(0)[...] = np.random.RandomState(1).uniform(-1, 1, net.shape(0)).astype(np.float32)
        net.upload(0)
        _trace_start()
        net.forward()
        net.sync()
        assert _trace_stop().count(BF16_FAMILY) == 1
    net.close()
