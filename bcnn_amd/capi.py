"""ctypes binding of lib/libbcnn.so -- the C99 host runtime (bcnn_net / bcnn_node API of include/bcnn/bcnn.h)
on top of the HIP back-end. Mirrors the reference's public API one to one; `Net` is a thin convenience
wrapper used by tests and bench.py (same method names as oracle/ref_bind.RefNet, which drives the
unmodified reference, so a graph can be built on both with the same code)."""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("BCNN_LIB", os.path.join(_HERE, "lib", "libbcnn.so"))  # override: experiment build

MODE_PREDICT, MODE_TRAIN, MODE_VALID = 0, 1, 2
PRECISION_FP32, PRECISION_BF16 = 0, 1
(ACT_NONE, ACT_TANH, ACT_RELU, ACT_RAMP, ACT_SOFTPLUS, ACT_LRELU, ACT_ABS, ACT_CLAMP, ACT_PRELU,
 ACT_LOGISTIC, ACT_RELU6, ACT_HARD_SIGMOID, ACT_HARD_SWISH, ACT_SWISH, ACT_MISH) = range(15)
PADDING_SAME, PADDING_VALID, PADDING_CAFFE = 0, 1, 2
FILLER_FIXED, FILLER_XAVIER, FILLER_MSRA = 0, 1, 2
LOSS_EUCLIDEAN, LOSS_LIFTED_STRUCT = 0, 1
LOG_SILENT = 3
(LOAD_MNIST, LOAD_CIFAR10, LOAD_CLASSIFICATION_LIST, LOAD_REGRESSION_LIST, LOAD_DETECTION_LIST) = range(5)
LOAD_SEGMENTATION_LIST = 6  # BCNN_NUM_LOADERS + 1: a constant behind the enumerator list (bcnn.h)
IMAGE_FIT_STRETCH, IMAGE_FIT_LETTERBOX = 0, 1
POOL2D_MAX, POOL2D_AVG = 0, 1
LAYER_ACTIVATION, LAYER_POOL2D, LAYER_SCALE_CHANNELS, LAYER_GROUPNORM = 3, 17, 18, 19
LAYER_CONV2D, LAYER_BATCHNORM, LAYER_DILATED_CONV2D, LAYER_INTERP = 0, 9, 20, 21
LAYER_SOFTMAX_LOSS = 22
LAYER_DEPTHWISE_CONV2D, LAYER_DILATED_DEPTHWISE_CONV2D = 2, 23
LOSS_NORM_NONE, LOSS_NORM_VALID, LOSS_NORM_VALID_PER_IMAGE = 0, 1, 2
LOSS_NORMS = {"none": LOSS_NORM_NONE, "valid": LOSS_NORM_VALID, "valid_per_image": LOSS_NORM_VALID_PER_IMAGE}


class Tensor(C.Structure):
    """struct bcnn_tensor with BCNN_USE_HIP (include/bcnn/bcnn.h)."""
    _fields_ = [("n", C.c_int), ("c", C.c_int), ("h", C.c_int), ("w", C.c_int), ("has_grad", C.c_int),
                ("name", C.c_char_p), ("data", C.POINTER(C.c_float)), ("grad_data", C.POINTER(C.c_float)),
                ("data_gpu", C.c_void_p), ("grad_data_gpu", C.c_void_p)]


class Detection(C.Structure):
    """struct bcnn_output_detection (include/bcnn/bcnn.h); prob / mask / the array itself come from calloc."""
    _fields_ = [("num_classes", C.c_int), ("x", C.c_float), ("y", C.c_float), ("w", C.c_float), ("h", C.c_float),
                ("prob", C.POINTER(C.c_float)), ("mask", C.POINTER(C.c_float)), ("objectness", C.c_float)]


class YoloTrainStats(C.Structure):
    """struct bcnn_yolo_train_stats (include/bcnn/bcnn.h)."""
    _fields_ = [("avg_iou", C.c_float), ("avg_class", C.c_float), ("avg_obj", C.c_float), ("avg_anyobj", C.c_float),
                ("recall50", C.c_float), ("recall75", C.c_float), ("count", C.c_int), ("cost", C.c_float)]


class LabelMapEval(C.Structure):
    """struct bcnn_label_map_eval (include/bcnn/bcnn.h)."""
    _fields_ = [("truths", C.POINTER(C.c_void_p)), ("strides", C.POINTER(C.c_int)), ("ignore_label", C.c_int),
                ("counts", C.POINTER(C.c_int64)), ("ignored", C.c_int64), ("out_of_range", C.c_int64)]


def iou_from_confusion(counts):
    """per-class IoU and their mean from a C x C confusion matrix (row = truth, column = label):
    IoU_k = counts[k][k] / (row sum k + column sum k - counts[k][k]); NaN for a class that is absent from both the truths
    and the labels, which the mean skips (NaN when every class is absent)"""
    m = np.asarray(counts, dtype=np.float64)
    assert m.ndim == 2 and m.shape[0] == m.shape[1], "a square matrix"
    inter = np.diag(m)
    union = m.sum(0) + m.sum(1) - inter
    iou = np.where(union > 0, inter / np.where(union > 0, union, 1.0), np.nan)
    return iou, (float(np.nanmean(iou)) if (union > 0).any() else float("nan"))


class SoftmaxLossStats(C.Structure):
    """struct bcnn_softmax_loss_stats (include/bcnn/bcnn.h)."""
    _fields_ = [("loss", C.c_float), ("valid", C.c_int64), ("ignored", C.c_int64), ("out_of_range", C.c_int64),
                ("correct", C.c_int64)]


_libc = C.CDLL(None)
_libc.free.argtypes, _libc.free.restype = [C.c_void_p], None


def detections_to_list(dets, count):
    """copies a bcnn_yolo_get_detections result into dicts (x, y, w, h, objectness, prob) and frees it as a C caller
    would: free(prob), free(mask), free(array)"""
    out = []
    if not dets:
        return out
    for k in range(count):
        d = dets[k]
        out.append(dict(x=d.x, y=d.y, w=d.w, h=d.h, objectness=d.objectness,
                        prob=np.array(d.prob[:d.num_classes], np.float32)))
        _libc.free(C.cast(d.prob, C.c_void_p))
        _libc.free(C.cast(d.mask, C.c_void_p))
    _libc.free(C.cast(dets, C.c_void_p))
    return out


def detections_batch_to_lists(L, dets, counts):
    """copies a bcnn_yolo_get_detections_batch result (per-image arrays and counts) into one list of dicts per image and
    frees every array through bcnn_free_detections"""
    out = []
    for b in range(len(counts)):
        out.append([dict(x=d.x, y=d.y, w=d.w, h=d.h, objectness=d.objectness,
                         prob=np.array(d.prob[:d.num_classes], np.float32))
                    for d in (dets[b][k] for k in range(counts[b]))] if dets[b] else [])
        L.bcnn_free_detections(dets[b], counts[b])
    return out


_lib = None


def build():
    from . import _lib as hip
    hip.build()
    subprocess.check_call(["make", "-C", os.path.join(_HERE, "host")], stdout=subprocess.DEVNULL)


def lib():
    global _lib
    if _lib is not None:
        return _lib
    from . import _lib as hip
    hip.load()  # loads libbcnn_hip.so first (and torch before it, see _lib.load)
    if not os.path.exists(LIB_PATH):
        raise RuntimeError("bcnn_amd: %s missing -- run __graft_entry__.build()" % LIB_PATH)
    L = C.CDLL(LIB_PATH)
    vp, i, f, cp, sz = C.c_void_p, C.c_int, C.c_float, C.c_char_p, C.c_size_t
    tp = C.POINTER(Tensor)
    sig = {
        "bcnn_init_net": (i, [C.POINTER(vp), i]), "bcnn_end_net": (None, [C.POINTER(vp)]),
        "bcnn_set_log_context": (None, [vp, vp, i]), "bcnn_set_input_shape": (None, [vp, i, i, i, i]),
        "bcnn_compile_net": (i, [vp]), "bcnn_set_mode": (i, [vp, i]), "bcnn_resize_net": (i, [vp, i, i, i, i]),
        "bcnn_forward": (None, [vp]), "bcnn_backward": (None, [vp]), "bcnn_update": (None, [vp]),
        "bcnn_train_on_batch": (f, [vp]),
        "bcnn_set_sgd_optimizer": (None, [vp, f, f]), "bcnn_set_weight_regularizer": (None, [vp, f]),
        "bcnn_get_tensor_index_by_name": (i, [vp, cp]), "bcnn_get_tensor_by_index": (tp, [vp, i]),
        "bcnn_get_batch_size": (i, [vp]),
        "bcnn_add_convolutional_layer": (i, [vp, i, i, i, i, i, i, i, i, i, cp, cp]),
        "bcnn_add_depthwise_conv_layer": (i, [vp, i, i, i, i, i, i, cp, cp]),
        "bcnn_add_deconvolutional_layer": (i, [vp, i, i, i, i, i, i, cp, cp]),
        "bcnn_add_dilated_conv_layer": (i, [vp, i, i, i, i, i, i, i, i, cp, cp]),
        "bcnn_add_dilated_depthwise_conv_layer": (i, [vp, i, i, i, i, i, i, cp, cp]),
        "bcnn_add_interp_layer": (i, [vp, i, i, i, i, i, cp, cp]),
        "bcnn_add_softmax_loss_layer": (i, [vp, i, i, f, cp, cp, cp]),
        "bcnn_get_softmax_loss_stats": (i, [vp, i, C.POINTER(SoftmaxLossStats)]),
        "bcnn_get_confusion_matrix": (i, [vp, i, C.POINTER(C.c_int64)]),
        "bcnn_get_label_maps_batch": (i, [vp, i, i, C.POINTER(i), C.POINTER(i), i, i, C.POINTER(vp), C.POINTER(i),
                                          C.POINTER(LabelMapEval)]),
        "bcnn_add_lrn_layer": (i, [vp, i, f, f, f, cp, cp]), "bcnn_add_dropout_layer": (i, [vp, f, cp]),
        "bcnn_set_dropout_seed": (None, [vp, C.c_uint64]),
        "bcnn_get_lifted_struct_loss": (i, [vp, C.POINTER(f), C.POINTER(i)]),
        "bcnn_add_batchnorm_layer": (i, [vp, cp, cp]), "bcnn_add_maxpool_layer": (i, [vp, i, i, i, cp, cp]),
        "bcnn_add_avgpool_layer": (i, [vp, cp, cp]), "bcnn_add_activation_layer": (i, [vp, i, cp]),
        "bcnn_add_pool2d_layer": (i, [vp, i, i, i, i, i, i, cp, cp]),
        "bcnn_add_scale_channels_layer": (i, [vp, cp, cp, cp]),
        "bcnn_add_groupnorm_layer": (i, [vp, i, f, cp, cp]),
        "bcnn_add_eltwise_layer": (i, [vp, i, cp, cp, cp]), "bcnn_add_fullc_layer": (i, [vp, i, i, i, i, cp, cp]),
        "bcnn_add_softmax_layer": (i, [vp, cp, cp]), "bcnn_add_cost_layer": (i, [vp, i, i, f, cp, cp, cp]),
        "bcnn_upload_tensor": (i, [vp, i, i]), "bcnn_download_tensor": (i, [vp, i, i]),
        "bcnn_set_data_parallel": (i, [vp, i, i]), "bcnn_set_data_parallel_comm": (i, [vp, i, i, cp]),
        "bcnn_set_weight_gradient_stream": (None, [vp, i]),
        "bcnn_set_inference_precision": (i, [vp, i]), "bcnn_get_inference_precision": (i, [vp]),
        "bcnn_set_loader_on_device": (i, [vp, i]), "bcnn_get_loader_on_device": (i, [vp]),
        "bcnn_set_loader_decode_on_device": (i, [vp, i]), "bcnn_get_loader_decode_on_device": (i, [vp]),
        "bcnn_get_loader_device_decoded": (i, [vp]),
        "bcnn_set_loader_detection_on_device": (i, [vp, i]), "bcnn_get_loader_detection_on_device": (i, [vp]),
        "bcnn_get_loader_device_letterboxed": (i, [vp]),
        "bcnn_get_loader_device_labels": (i, [vp]), "bcnn_loader_next": (i, [vp]),
        "bcnn_set_loader_effects": (i, [vp, i]), "bcnn_get_loader_effects": (i, [vp]),
        "bcnn_set_detector_training": (i, [vp, i]), "bcnn_get_detector_training": (i, [vp]),
        "bcnn_yolo_get_train_stats": (i, [vp, i, C.POINTER(YoloTrainStats)]),
        "bcnn_set_data_loader": (i, [vp, i, cp, cp, cp, cp]),
        "bcnn_set_gradient_ready_callback": (None, [vp, vp, vp]),
        "bcnn_get_gradient_arena": (vp, [vp, C.POINTER(sz)]), "bcnn_get_parameter_arena": (vp, [vp, C.POINTER(sz)]),
        "bcnn_synchronize": (None, [vp]), "bcnn_peek_tensor": (tp, [vp, i]), "bcnn_get_num_nodes": (i, [vp]),
        "bcnn_get_node_tensor": (i, [vp, i, i, i]), "bcnn_get_node_state": (vp, [vp, i, i]),
        "bcnn_get_node_type": (i, [vp, i]), "bcnn_get_node_activation": (i, [vp, i]),
        "bcnn_forward_node": (i, [vp, i]), "bcnn_backward_node": (i, [vp, i]),
        "bcnn_load_net": (i, [vp, cp, cp]), "bcnn_save_weights": (i, [vp, cp]), "bcnn_load_weights": (i, [vp, cp]),
        "bcnn_add_concat_layer": (i, [vp, i, C.POINTER(cp), cp]), "bcnn_add_upsample_layer": (i, [vp, i, cp, cp]),
        "bcnn_add_yolo_layer": (i, [vp, i, i, i, i, C.POINTER(i), C.POINTER(f), cp, cp]),
        "bcnn_yolo_get_detections": (C.POINTER(Detection), [vp, i, i, i, i, i, f, i, C.POINTER(i)]),
        "bcnn_yolo_get_detections_batch": (i, [vp, C.POINTER(i), C.POINTER(i), i, i, f, i,
                                               C.POINTER(C.POINTER(Detection)), C.POINTER(i)]),
        "bcnn_free_detections": (None, [C.POINTER(Detection), i]),
        "bcnn_fill_tensor_with_images": (i, [vp, i, i, C.POINTER(vp), C.POINTER(i), C.POINTER(i), C.POINTER(i), i, i, f,
                                             i, f, f, f]),
        "bcnn_fill_tensor_with_jpegs": (i, [vp, i, i, C.POINTER(vp), C.POINTER(sz), i, f, i, f, f, f, C.POINTER(i)]),
        "bcnn_set_num_threads": (i, [vp, i, C.POINTER(i)]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(L, name)
        fn.restype, fn.argtypes = res, args
    _lib = L
    return L


class DeviceArray:
    """Exposes a raw device pointer through __cuda_array_interface__ so torch.as_tensor can alias it."""

    def __init__(self, ptr, n):
        self.__cuda_array_interface__ = {"shape": (int(n),), "typestr": "<f4", "data": (int(ptr), False),
                                         "version": 2, "strides": None}


class Net:
    def __init__(self, mode=MODE_TRAIN, w=8, h=8, c=3, n=2, input_grad=False, silent=True):
        self.L = lib()
        self.net = C.c_void_p()
        assert self.L.bcnn_init_net(C.byref(self.net), mode) == 0
        if silent:
            self.L.bcnn_set_log_context(self.net, None, LOG_SILENT)
        self.L.bcnn_set_input_shape(self.net, w, h, c, n)
        self.num_nodes = 0
        self._node_io = []
        if input_grad:
            self.tensor(0).has_grad = 1

    # builders return the node index, like ref_bind.RefNet
    def _added(self, st):
        assert st == 0, "builder failed with status %d" % st
        self.num_nodes += 1
        return self.num_nodes - 1

    def conv(self, f, k, s, p, g=1, bn=0, act=ACT_NONE, src="input", dst="conv", init=FILLER_XAVIER):
        return self._added(self.L.bcnn_add_convolutional_layer(self.net, f, k, s, p, g, bn, init, act, 0,
                                                                src.encode(), dst.encode()))

    def deconv(self, f, k, s, p, act=ACT_NONE, src="input", dst="deconv", init=FILLER_XAVIER):
        """bcnn_add_deconvolutional_layer: f output channels, k x k kernel, stride s, pad p"""
        return self._added(self.L.bcnn_add_deconvolutional_layer(self.net, f, k, s, p, init, act, src.encode(),
                                                                  dst.encode()))

    def dilated_conv(self, f, k, s, p, d, g=1, act=ACT_NONE, src="input", dst="dconv", init=FILLER_XAVIER):
        """bcnn_add_dilated_conv_layer: f filters, k x k kernel with taps d apart, stride s, pad p, g groups; d == 1
        builds an ordinary convolution node"""
        return self._added(self.L.bcnn_add_dilated_conv_layer(self.net, f, k, s, p, d, g, init, act, src.encode(),
                                                               dst.encode()))

    def lrn(self, local_size, alpha, beta, k=1.0, src="input", dst="lrn"):
        """bcnn_add_lrn_layer: local response normalisation across channels"""
        return self._added(self.L.bcnn_add_lrn_layer(self.net, local_size, alpha, beta, k, src.encode(), dst.encode()))

    def dropout(self, rate, src):
        """bcnn_add_dropout_layer: in place on tensor `src`"""
        return self._added(self.L.bcnn_add_dropout_layer(self.net, rate, src.encode()))

    def depthwise(self, k, s, p, act=ACT_NONE, src="input", dst="dw"):
        return self._added(self.L.bcnn_add_depthwise_conv_layer(self.net, k, s, p, 0, FILLER_XAVIER, act,
                                                                 src.encode(), dst.encode()))

    def dilated_depthwise(self, k, s, p, d, act=ACT_NONE, src="input", dst="ddw", init=FILLER_XAVIER):
        """bcnn_add_dilated_depthwise_conv_layer: one k x k filter per channel with taps d apart, stride s, pad p; d == 1
        builds an ordinary depthwise node"""
        return self._added(self.L.bcnn_add_dilated_depthwise_conv_layer(self.net, k, s, p, d, init, act, src.encode(),
                                                                         dst.encode()))

    def batchnorm(self, src, dst):
        return self._added(self.L.bcnn_add_batchnorm_layer(self.net, src.encode(), dst.encode()))

    def maxpool(self, k, s, padding=PADDING_SAME, src="input", dst="pool"):
        return self._added(self.L.bcnn_add_maxpool_layer(self.net, k, s, padding, src.encode(), dst.encode()))

    def avgpool(self, src, dst):
        return self._added(self.L.bcnn_add_avgpool_layer(self.net, src.encode(), dst.encode()))

    def pool2d(self, kind, size, stride, pad=0, ceil_mode=False, count_include_pad=True, src="input", dst="pool"):
        """bcnn_add_pool2d_layer: POOL2D_MAX / POOL2D_AVG (or "max" / "avg") over a size x size window, `stride` apart,
        `pad` on all four sides -- the rules of torch's max_pool2d / avg_pool2d"""
        kind = {"max": POOL2D_MAX, "avg": POOL2D_AVG}.get(kind, kind)
        return self._added(self.L.bcnn_add_pool2d_layer(self.net, kind, size, stride, pad, 1 if ceil_mode else 0,
                                                         1 if count_include_pad else 0, src.encode(), dst.encode()))

    def scale_channels(self, src, gate, dst):
        """bcnn_add_scale_channels_layer: dst = src * gate, gate [N,C,1,1] (squeeze-and-excitation) or src's shape (sam)"""
        return self._added(self.L.bcnn_add_scale_channels_layer(self.net, src.encode(), gate.encode(), dst.encode()))

    def groupnorm(self, groups, src, dst, eps=0.0):
        """bcnn_add_groupnorm_layer: group normalisation over `groups` groups of channels (1: layer norm over (C,H,W),
        C: instance norm with affine); eps <= 0 selects 1e-5"""
        return self._added(self.L.bcnn_add_groupnorm_layer(self.net, groups, eps, src.encode(), dst.encode()))

    def activation(self, act, src):
        return self._added(self.L.bcnn_add_activation_layer(self.net, act, src.encode()))

    def eltwise(self, act, src1, src2, dst):
        return self._added(self.L.bcnn_add_eltwise_layer(self.net, act, src1.encode(), src2.encode(), dst.encode()))

    def fullc(self, out, act=ACT_NONE, src="input", dst="fc"):
        return self._added(self.L.bcnn_add_fullc_layer(self.net, out, FILLER_XAVIER, act, 0, src.encode(), dst.encode()))

    def softmax(self, src, dst):
        return self._added(self.L.bcnn_add_softmax_layer(self.net, src.encode(), dst.encode()))

    def cost(self, src, label="label", dst="cost", scale=1.0, loss=LOSS_EUCLIDEAN, metric=0):
        return self._added(self.L.bcnn_add_cost_layer(self.net, loss, metric, scale, src.encode(), label.encode(),
                                                      dst.encode()))

    def lifted_struct_loss(self):
        """(loss, positive pairs) of the latest forward of the net's last lifted-structure cost node"""
        loss, pairs = C.c_float(), C.c_int()
        st = self.L.bcnn_get_lifted_struct_loss(self.net, C.byref(loss), C.byref(pairs))
        if st != 0:
            raise ValueError("the net has no lifted-structure cost node (status %d)" % st)
        return loss.value, pairs.value

    def concat(self, srcs, dst):
        """bcnn_add_concat_layer: srcs (tensor names) stacked along the channels"""
        arr = (C.c_char_p * len(srcs))(*[x.encode() for x in srcs])
        return self._added(self.L.bcnn_add_concat_layer(self.net, len(srcs), arr, dst.encode()))

    def upsample(self, size, src, dst):
        return self._added(self.L.bcnn_add_upsample_layer(self.net, size, src.encode(), dst.encode()))

    def interp(self, src, dst, scale=0, zoom=0, out_w=0, out_h=0, align_corners=False):
        """bcnn_add_interp_layer: bilinear interpolation to in * scale, to (in - 1) * zoom + 1 or to out_w x out_h (exactly
        one form) -- torch's interpolate(mode="bilinear", align_corners=...); Caffe-DeepLab's Interp is align_corners"""
        return self._added(self.L.bcnn_add_interp_layer(self.net, out_w, out_h, scale, zoom, 1 if align_corners else 0,
                                                        src.encode(), dst.encode()))

    def softmax_loss(self, src, dst, ignore_label=-1, normalize="valid_per_image", scale=1.0):
        """bcnn_add_softmax_loss_layer: softmax over the channels of src and cross-entropy against the class-index label
        map in tensor 1 ([n][1][h][w], floats); normalize: "none", "valid", "valid_per_image" or a LOSS_NORM_* value"""
        return self._added(self.L.bcnn_add_softmax_loss_layer(self.net, ignore_label, LOSS_NORMS.get(normalize, normalize),
                                                              scale, src.encode(), b"label", dst.encode()))

    def softmax_loss_stats(self, node):
        """bcnn_get_softmax_loss_stats of the node's latest TRAIN / VALID forward, as a dict (loss, valid, ignored,
        out_of_range, correct); raises ValueError when the node has none (not such a node, a PREDICT forward)"""
        out = SoftmaxLossStats()
        st = self.L.bcnn_get_softmax_loss_stats(self.net, node, C.byref(out))
        if st != 0:
            raise ValueError("node %d has no softmax-loss statistics (status %d)" % (node, st))
        return {name: getattr(out, name) for name, _ in SoftmaxLossStats._fields_}

    def confusion_matrix(self, node):
        """bcnn_get_confusion_matrix: the C x C int64 matrix (row = label, column = argmax) of the node's latest forward"""
        c = self.shape(self.node_dst(node))[1]
        counts = np.zeros((c, c), np.int64)
        st = self.L.bcnn_get_confusion_matrix(self.net, node, counts.ctypes.data_as(C.POINTER(C.c_int64)))
        if st != 0:
            raise ValueError("node %d has no confusion matrix (status %d)" % (node, st))
        return counts

    def yolo(self, num, classes, mask, anchors, src, dst, coords=4):
        """bcnn_add_yolo_layer: `mask` (num anchor indices), `anchors` (2 * total extents) or None (all 0.5 x total)"""
        m = (C.c_int * len(mask))(*mask) if mask is not None else None
        total = len(anchors) // 2 if anchors is not None else num
        a = (C.c_float * len(anchors))(*anchors) if anchors is not None else None
        return self._added(self.L.bcnn_add_yolo_layer(self.net, num, classes, coords, total, m, a, src.encode(),
                                                       dst.encode()))

    def get_detections(self, batch, w, h, netw, neth, thresh, relative):
        """bcnn_yolo_get_detections, as a list of dicts (count includes the boxes NMS suppressed: objectness 0)"""
        n = C.c_int(0)
        dets = self.L.bcnn_yolo_get_detections(self.net, batch, w, h, netw, neth, thresh, relative, C.byref(n))
        return detections_to_list(dets, n.value)

    def get_detections_batch(self, sizes, netw, neth, thresh, relative):
        """bcnn_yolo_get_detections_batch: `sizes` holds the original (w, h) of every image of the batch; returns one
        list of dicts per image, each like get_detections (equal objectness: by candidate index, see bcnn.h)"""
        n = len(sizes)
        assert n == self.L.bcnn_get_batch_size(self.net), "one (w, h) per image of the batch"
        ws, hs = (C.c_int * n)(*[s[0] for s in sizes]), (C.c_int * n)(*[s[1] for s in sizes])
        dets, counts = (C.POINTER(Detection) * n)(), (C.c_int * n)()
        st = self.L.bcnn_yolo_get_detections_batch(self.net, ws, hs, netw, neth, thresh, relative, dets, counts)
        if st != 0:
            raise ValueError("bcnn_yolo_get_detections_batch failed with status %d" % st)
        return detections_batch_to_lists(self.L, dets, counts)

    @classmethod
    def load_net(cls, config_path, model_path=None, mode=MODE_PREDICT, silent=True):
        """bcnn_load_net (bcnn or Darknet config dialect; a *.weights model selects Darknet); raises on failure"""
        net = cls.__new__(cls)
        net.L, net.net, net._node_io = lib(), C.c_void_p(), []
        assert net.L.bcnn_init_net(C.byref(net.net), mode) == 0
        if silent:
            net.L.bcnn_set_log_context(net.net, None, LOG_SILENT)
        st = net.L.bcnn_load_net(net.net, config_path.encode(), model_path.encode() if model_path else None)
        if st != 0:
            net.close()
            raise RuntimeError("bcnn_load_net(%s) failed with status %d" % (config_path, st))
        net.num_nodes = net.L.bcnn_get_num_nodes(net.net)
        return net

    def set_mode(self, mode):
        return self.L.bcnn_set_mode(self.net, mode)

    def set_inference_precision(self, precision):
        """bcnn_set_inference_precision: PRECISION_BF16 runs every convolution node of a PREDICT / VALID forward on the
        bf16 matrix cores (fp32 accumulator; depthwise (dilated or not), deconvolution, dilated-convolution and full-connected nodes stay fp32); a TRAIN-mode
        pass is never affected. Returns the bcnn_status (1 = BCNN_INVALID_PARAMETER for an unknown value)."""
        return self.L.bcnn_set_inference_precision(self.net, precision)

    def get_inference_precision(self):
        return self.L.bcnn_get_inference_precision(self.net)

    def set_loader_on_device(self, on):
        """bcnn_set_loader_on_device: bcnn_loader_next makes the input batch on the device from the raw uint8 samples
        (augmentation, centre crop and conversion; bit-identical to the host path). The host copy of tensor 0 is then not
        written: download(0) refreshes it. Returns the bcnn_status."""
        return self.L.bcnn_set_loader_on_device(self.net, 1 if on else 0)

    def get_loader_on_device(self):
        return self.L.bcnn_get_loader_on_device(self.net)

    def set_loader_decode_on_device(self, on):
        """bcnn_set_loader_decode_on_device: with set_loader_on_device, the JPEG entries of a classification / regression
        list are entropy-decoded on the host (on set_num_threads() threads) and become pixels, cropped to the net input,
        on the device only; every other entry is decoded on the host as before. Same batch, bit for bit. Returns the
        bcnn_status."""
        return self.L.bcnn_set_loader_decode_on_device(self.net, 1 if on else 0)

    def get_loader_decode_on_device(self):
        return self.L.bcnn_get_loader_decode_on_device(self.net)

    def loader_device_decoded(self):
        """bcnn_get_loader_device_decoded: samples of the latest bcnn_loader_next whose pixels were decoded on the device"""
        return self.L.bcnn_get_loader_device_decoded(self.net)

    def set_loader_detection_on_device(self, on):
        """bcnn_set_loader_detection_on_device: with set_loader_on_device, a detection-list batch is resized, pasted on
        its grey canvas, augmented and converted on the device; the host decodes the files (on set_num_threads() threads),
        makes the draws and writes the labels. Same batch, labels and rand() state, bit for bit. Returns the bcnn_status."""
        return self.L.bcnn_set_loader_detection_on_device(self.net, 1 if on else 0)

    def get_loader_detection_on_device(self):
        return self.L.bcnn_get_loader_detection_on_device(self.net)

    def loader_device_letterboxed(self):
        """bcnn_get_loader_device_letterboxed: samples of the latest bcnn_loader_next that were letterboxed on the device"""
        return self.L.bcnn_get_loader_device_letterboxed(self.net)

    def set_data_loader(self, kind, train, train_extra=None, test=None, test_extra=None):
        """bcnn_set_data_loader: opens the train / test streams of one of the LOAD_* formats; returns the status.
        LOAD_SEGMENTATION_LIST ("image-path mask-path" lines) needs a softmax-loss node in the net."""
        enc = lambda s: s.encode() if s else None
        return self.L.bcnn_set_data_loader(self.net, kind, enc(train), enc(train_extra), enc(test), enc(test_extra))

    def loader_next(self):
        """bcnn_loader_next: one batch into tensors 0 and 1 (host and device); returns the status"""
        return self.L.bcnn_loader_next(self.net)

    def loader_device_labels(self):
        """bcnn_get_loader_device_labels: label maps of the latest bcnn_loader_next that were made on the device"""
        return self.L.bcnn_get_loader_device_labels(self.net)

    def set_loader_effects(self, on):
        """bcnn_set_loader_effects: bcnn_loader_next applies Perlin distortion (max_distortion) and random spotlights
        (max_spots) to TRAIN samples, on the host path and on every device route, bit for bit like the reference; off
        (the default) their rand() draws are made and the pixels stay. Returns the bcnn_status."""
        return self.L.bcnn_set_loader_effects(self.net, 1 if on else 0)

    def get_loader_effects(self):
        return self.L.bcnn_get_loader_effects(self.net)

    def set_detector_training(self, on):
        """bcnn_set_detector_training: YOLO heads may be built on a TRAIN net (or switched to TRAIN), their TRAIN forward
        computes the YOLOv3 loss gradient on the device and the detection-list loader is accepted. Set it before the
        heads are built. Returns the bcnn_status."""
        return self.L.bcnn_set_detector_training(self.net, 1 if on else 0)

    def get_detector_training(self):
        return self.L.bcnn_get_detector_training(self.net)

    def yolo_train_stats(self, node):
        """bcnn_yolo_get_train_stats of YOLO node `node` after a TRAIN forward, as a dict (avg_iou, avg_class, avg_obj,
        avg_anyobj, recall50, recall75, count, cost); raises ValueError for a node that is no YOLO head"""
        out = YoloTrainStats()
        st = self.L.bcnn_yolo_get_train_stats(self.net, node, C.byref(out))
        if st != 0:
            raise ValueError("node %d is not a YOLO head (status %d)" % (node, st))
        return {name: getattr(out, name) for name, _ in YoloTrainStats._fields_}

    def compile(self):
        assert self.L.bcnn_compile_net(self.net) == 0

    def resize(self, w, h, c, need_realloc=True):
        """bcnn_resize_net (reference bcnn_net.c:287-335): batch 1, destination tensors re-shaped (and re-allocated)"""
        return self.L.bcnn_resize_net(self.net, w, h, c, 1 if need_realloc else 0)

    # tensors: host views; call download()/upload() around them
    def index(self, name):
        return self.L.bcnn_get_tensor_index_by_name(self.net, name.encode())

    def tensor(self, idx):
        # raw struct WITHOUT the implicit device->host refresh of bcnn_get_tensor_by_index
        return self.L.bcnn_peek_tensor(self.net, idx).contents

    def node_src(self, node, i):
        return self.L.bcnn_get_node_tensor(self.net, node, 0, i)

    def node_dst(self, node, i=0):
        return self.L.bcnn_get_node_tensor(self.net, node, 1, i)

    def node_type(self, node):
        return int(self.L.bcnn_get_node_type(self.net, node))

    def node_activation(self, node):
        """the bcnn_activation of a node that has one, else -1"""
        return int(self.L.bcnn_get_node_activation(self.net, node))

    def node_state(self, node, which):
        return self.L.bcnn_get_node_state(self.net, node, which)

    def shape(self, idx):
        t = self.tensor(idx)
        return (t.n, t.c, t.h, t.w)

    def _view(self, ptr, shape):
        return np.ctypeslib.as_array(ptr, shape=(int(np.prod(shape)),)).reshape(shape)

    def data(self, idx):
        t = self.tensor(idx)
        return self._view(t.data, (t.n, t.c, t.h, t.w))

    def grad(self, idx):
        t = self.tensor(idx)
        return self._view(t.grad_data, (t.n, t.c, t.h, t.w)) if t.grad_data else None

    def upload(self, idx, with_grad=False):
        assert self.L.bcnn_upload_tensor(self.net, idx, 1 if with_grad else 0) == 0

    def download(self, idx, with_grad=True):
        assert self.L.bcnn_download_tensor(self.net, idx, 1 if with_grad else 0) == 0

    def fill_images(self, images, fit=IMAGE_FIT_STRETCH, norm_coeff=1.0, swap_to_bgr=False, mean=(0.0, 0.0, 0.0),
                    tensor=0):
        """bcnn_fill_tensor_with_images: `images` is a list of H x W x C uint8 arrays (H x W for one channel), one per
        batch entry from 0 on; each is resized (or letterboxed) to the tensor's extent and converted on the device.
        Rows that are not contiguous go through `strides`; only an array whose pixels are not contiguous is copied.
        Returns the bcnn_status (1 = BCNN_INVALID_PARAMETER: the tensor is untouched)."""
        keep, ptrs, ws, hs, ss = [], [], [], [], []
        c = None
        for im in images:
            a = np.asarray(im)
            assert a.dtype == np.uint8 and a.ndim in (2, 3), "H x W x C uint8 arrays"
            if a.ndim == 2:
                a = a[:, :, None]
            ch = a.shape[2]
            if a.size and (a.strides[2] != 1 or a.strides[1] != ch or a.strides[0] < a.shape[1] * ch):
                a = np.ascontiguousarray(a)
            assert c is None or c == ch, "all images have the same number of channels"
            c = ch
            keep.append(a)
            ptrs.append(a.ctypes.data if a.size else None)
            hs.append(a.shape[0])
            ws.append(a.shape[1])
            ss.append(a.strides[0] if a.size else a.shape[1] * ch)
        k = len(keep)
        return self.L.bcnn_fill_tensor_with_images(self.net, tensor, k, (C.c_void_p * k)(*ptrs), (C.c_int * k)(*ws),
                                                   (C.c_int * k)(*hs), (C.c_int * k)(*ss), c if c is not None else 0,
                                                   fit, norm_coeff, 1 if swap_to_bgr else 0, mean[0], mean[1], mean[2])

    def label_maps(self, tensor, sizes, fit=IMAGE_FIT_STRETCH, align_corners=False, truths=None, ignore_label=255,
                   labels=True):
        """bcnn_get_label_maps_batch: one uint8 array [h][w] of class indices per (w, h) of `sizes` (the original sizes of
        the images the batch was filled with, with the same `fit`), from tensor `tensor` ([n][C][h][w] logits or
        probabilities). With `truths` (uint8 arrays of those sizes) returns (labels, counts, ignored, out_of_range), counts
        the C x C int64 matrix (row = truth, column = label); labels=False skips the label maps (None in their place).
        Raises ValueError with the bcnn_status when the library refuses."""
        k = len(sizes)
        ws, hs = (C.c_int * max(k, 1))(*[int(s[0]) for s in sizes]), (C.c_int * max(k, 1))(*[int(s[1]) for s in sizes])
        out = [np.empty((int(s[1]), int(s[0])), np.uint8) for s in sizes] if labels else None
        lptr = (C.c_void_p * max(k, 1))(*[a.ctypes.data for a in out]) if labels else None
        ev = None
        if truths is not None:
            keep = [np.ascontiguousarray(t, dtype=np.uint8) for t in truths]
            assert len(keep) == k and all(t.shape == (int(s[1]), int(s[0])) for t, s in zip(keep, sizes))
            c = self.shape(tensor)[1]
            counts = np.zeros((c, c), np.int64)
            tptr = (C.c_void_p * max(k, 1))(*[t.ctypes.data for t in keep])
            ev = LabelMapEval(tptr, None, int(ignore_label), counts.ctypes.data_as(C.POINTER(C.c_int64)), 0, 0)
        st = self.L.bcnn_get_label_maps_batch(self.net, tensor, k, ws, hs, fit, 1 if align_corners else 0, lptr, None,
                                              C.byref(ev) if ev is not None else None)
        if st != 0:
            raise ValueError("bcnn_get_label_maps_batch failed with status %d" % st)
        if ev is None:
            return out
        return out, counts, int(ev.ignored), int(ev.out_of_range)

    def fill_jpegs(self, jpegs, fit=IMAGE_FIT_STRETCH, norm_coeff=1.0, swap_to_bgr=False, mean=(0.0, 0.0, 0.0),
                   tensor=0, num_images=None):
        """bcnn_fill_tensor_with_jpegs: `jpegs` is a list of bytes objects, one JPEG stream per batch entry from 0 on;
        each is entropy-decoded on the host and turned into pixels, resized (or letterboxed) and converted on the
        device. Returns (bcnn_status, failed_image): (1, index) = BCNN_INVALID_PARAMETER, the tensor is untouched.
        `num_images` overrides the count passed to the library (tests of the refusals)."""
        keep = [np.frombuffer(bytes(j), np.uint8) for j in jpegs]
        k = len(keep)
        ptrs = (C.c_void_p * max(k, 1))(*[a.ctypes.data if a.size else None for a in keep])
        lens = (C.c_size_t * max(k, 1))(*[a.size for a in keep])
        failed = C.c_int(-1)
        st = self.L.bcnn_fill_tensor_with_jpegs(self.net, tensor, k if num_images is None else num_images, ptrs, lens, fit,
                                                norm_coeff, 1 if swap_to_bgr else 0, mean[0], mean[1], mean[2],
                                                C.byref(failed))
        return st, failed.value

    def set_num_threads(self, num_threads):
        """bcnn_set_num_threads: host threads of the calls that use them (bcnn_fill_tensor_with_jpegs)"""
        return self.L.bcnn_set_num_threads(self.net, num_threads, None)

    def forward(self):
        self.L.bcnn_forward(self.net)

    def backward(self):
        self.L.bcnn_backward(self.net)

    def update(self):
        self.L.bcnn_update(self.net)

    def forward_node(self, node):
        assert self.L.bcnn_forward_node(self.net, node) == 0

    def backward_node(self, node):
        assert self.L.bcnn_backward_node(self.net, node) == 0

    def sync(self):
        self.L.bcnn_synchronize(self.net)

    def save_weights(self, path):
        """bcnn_save_weights (reference bcnn_net.c:597-681); returns the bcnn_status"""
        return self.L.bcnn_save_weights(self.net, path.encode())

    def load_weights(self, path):
        """bcnn_load_weights (reference bcnn_net.c:1485-1558); returns the bcnn_status"""
        return self.L.bcnn_load_weights(self.net, path.encode())

    def set_sgd(self, lr, momentum, decay=0.0):
        self.L.bcnn_set_sgd_optimizer(self.net, lr, momentum)
        self.L.bcnn_set_weight_regularizer(self.net, decay)

    def set_data_parallel(self, rank, world):
        assert self.L.bcnn_set_data_parallel(self.net, rank, world) == 0

    def set_data_parallel_comm(self, rank, world, id_path=None):
        """RCCL inside the library: bcnn_backward all-reduces the gradient arena itself (include/bcnn/bcnn.h)"""
        assert self.L.bcnn_set_data_parallel_comm(self.net, rank, world, id_path.encode() if id_path else None) == 0

    def set_gradient_ready_callback(self, fn):
        """fn(first_float, num_floats) is called inside backward() as tail ranges of the gradient arena
        become final (see include/bcnn/bcnn.h); None removes it."""
        if fn is None:
            self._grad_cb = None
            self.L.bcnn_set_gradient_ready_callback(self.net, None, None)
            return
        proto = C.CFUNCTYPE(None, C.c_size_t, C.c_size_t, C.c_void_p)
        self._grad_cb = proto(lambda first, count, user: fn(int(first), int(count)))  # keep alive
        self.L.bcnn_set_gradient_ready_callback(self.net, C.cast(self._grad_cb, C.c_void_p), None)

    def gradient_arena(self):
        n = C.c_size_t()
        p = self.L.bcnn_get_gradient_arena(self.net, C.byref(n))
        return p, n.value

    def parameter_arena(self):
        n = C.c_size_t()
        p = self.L.bcnn_get_parameter_arena(self.net, C.byref(n))
        return p, n.value

    def close(self):
        if self.net:
            self.L.bcnn_end_net(C.byref(self.net))
            self.net = None
