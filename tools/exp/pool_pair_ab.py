"""usage: pool_pair_ab.py [act]. A/B of the two stem pooling kernels at the ResNet-18 shape on the experiment build: first generation (BCNN_HIP_POOL_PAIR_V1)
against the second, times from the library's own per-class event timer (class 'pool')."""
import ctypes, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
os.environ["BCNN_HIP_LIB"] = os.path.join(ROOT, "bcnn_amd", "lib", "libbcnn_hip_exp.so")
import torch
from bcnn_amd import _lib
L = _lib.load()
dev = "cuda:0"
n, c, h, w = 128, 64, 112, 112
oh, ow = 56, 56
act = int(sys.argv[1]) if len(sys.argv) > 1 else 2
torch.manual_seed(1)
x = torch.randn((n, c, h, w), device=dev)
mean, var = torch.randn(c, device=dev) * 0.1, torch.rand(c, device=dev) + 0.5
sc, b = torch.rand(c, device=dev) + 0.5, torch.randn(c, device=dev) * 0.1
yp = torch.empty((n, c, oh, ow), device=dev); idx = torch.empty((n, c, oh, ow), device=dev, dtype=torch.int32)
ram = torch.empty((n, c, oh, ow), device=dev); dpool = torch.randn((n, c, oh, ow), device=dev) * 0.1
g = torch.empty_like(x)
z = [torch.zeros(c, device=dev) for _ in range(4)]
P = lambda t: t.data_ptr()
POOL = [i for i in range(L.bcnn_hip_profile_num_classes()) if L.bcnn_hip_profile_class_name(i) == b"pool"][0]
def fwd(): L.bcnn_hip_maxpool_forward_bn_keep(P(x), P(yp), P(idx), n, c, h, w, oh, ow, 3, 2, P(sc), P(b), P(mean), P(var), act, P(ram))
def bwd(): L.bcnn_hip_maxpool_bn_backward(P(dpool), P(idx), P(ram), P(x), P(g), n, c, h, w, oh, ow, 3, 2, P(sc), P(z[0]), P(b), P(z[1]), P(mean), P(var), P(z[2]), P(z[3]), act)
def timed(fn, reps=20):
    for _ in range(3): fn()
    L.bcnn_hip_sync(); L.bcnn_hip_profile_enable(1); L.bcnn_hip_profile_reset()
    for _ in range(reps): fn()
    ms, k, by = ctypes.c_double(), ctypes.c_longlong(), ctypes.c_double()
    L.bcnn_hip_profile_read(POOL, ctypes.byref(ms), ctypes.byref(k), None, ctypes.byref(by))
    L.bcnn_hip_profile_enable(0); L.bcnn_hip_profile_reset()
    return ms.value / k.value * 1e3, by.value / k.value
keepres = {}
for rnd in range(3):
    for v1 in (True, False):
        if v1: os.environ["BCNN_HIP_POOL_PAIR_V1"] = "1"
        else: os.environ.pop("BCNN_HIP_POOL_PAIR_V1", None)
        for name, fn in (("fwd", fwd), ("bwd", bwd)):
            us, by = timed(fn)
            print("act%d round%d %s %s %.1f us  %.0f MB  %.2f TB/s" % (act, rnd, "v1" if v1 else "v2", name, us, by / 1e6, by / us / 1e6), flush=True)
        torch.cuda.synchronize()
        keepres[v1] = [t.clone() for t in (yp, idx, ram, g)]
print("bit-identical v1/v2:", [torch.equal(p.view(torch.int32), q.view(torch.int32)) for p, q in zip(keepres[True], keepres[False])])
