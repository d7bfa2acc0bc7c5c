"""The window-attention node under bcnn_set_inference_precision (bcnn_amd.capi): a PREDICT / VALID forward in bf16 runs
attention_window_bf16.hip, a TRAIN pass and an fp32 net run attention_window.hip; the dispatch trace says which. The net's data
are integers from {-1, 0, 1}, the q convolution's weights are zero and there is no bias table: every score is 0, the keys of a
region of 64, 32 or 16 positions weigh exactly 2^-6, 2^-5 or 2^-4 each, and both kernels give the same bits."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
FP32, BF16 = "window_attention_fwd", "window_attention_fwd_bf16"


def _net(mode):
    """input [2][4][16][16] -> three 1x1 convolutions q (8, zero weights), k (8), v (12) -> window attention, 2 heads, 8 x 8
    windows, shift 4"""
    from bcnn_amd import capi
    net = capi.Net(mode=mode, w=16, h=16, c=4, n=2)
    convs = [net.conv(f, 1, 1, 0, src="input", dst=name) for name, f in (("q", 8), ("k", 8), ("v", 12))]
    net.add_window_attention(2, 8, "q", "k", "v", "att", shift=4, rel_bias=False)
    net.compile()
    rs = np.random.RandomState(7)
    for i, zero in [(0, False)] + [(net.node_src(node, s), s == 2 or node == convs[0]) for node in convs for s in (1, 2)]:
        net.data(i)[...] = 0.0 if zero else rs.randint(-1, 2, net.shape(i)).astype(np.float32)
        net.upload(i)
    return net


def _forward(net):
    """(the node's output, the window-attention launches of the pass)"""
    from bcnn_amd import _lib
    L = _lib.load()
    L.bcnn_hip_trace_enable(1)
    net.forward()
    net.sync()
    n = L.bcnn_hip_trace_read(None, 0)
    buf = ctypes.create_string_buffer(n + 1)
    L.bcnn_hip_trace_read(buf, n + 1)
    L.bcnn_hip_trace_enable(0)
    att = net.index("att")
    net.download(att, with_grad=False)
    return net.data(att).copy().view(np.uint32), [name for name in buf.value.decode().split() if name.startswith(FP32)]


def test_predict_net_in_bf16_runs_the_bf16_kernel_and_gives_the_bits_of_fp32():
    from bcnn_amd import capi
    net = _net(capi.MODE_PREDICT)
    y32, names32 = _forward(net)
    assert names32 == [FP32] and y32.any()
    assert net.set_inference_precision(capi.PRECISION_BF16) == 0
    y16, names16 = _forward(net)
    assert names16 == [BF16] and np.array_equal(y16, y32)
    assert net.set_inference_precision(capi.PRECISION_FP32) == 0
    y32b, names32b = _forward(net)
    assert names32b == names32 and np.array_equal(y32b, y32)
    net.close()


def test_a_train_mode_pass_never_uses_it_and_set_mode_switches_it_on():
    from bcnn_amd import capi
    plain = _net(capi.MODE_TRAIN)
    y_plain, names_plain = _forward(plain)
    plain.close()
    net = _net(capi.MODE_TRAIN)
    assert net.set_inference_precision(capi.PRECISION_BF16) == 0
    y_train, names_train = _forward(net)
    assert names_train == names_plain == [FP32] and np.array_equal(y_train, y_plain)
    assert net.set_mode(capi.MODE_PREDICT) == 0
    y_pred, names_pred = _forward(net)
    assert names_pred == [BF16] and np.array_equal(y_pred, y_plain)
    net.close()
