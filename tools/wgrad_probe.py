#!/usr/bin/env python3
"""Time one windowed weight gradient through the C-ABI (optimisation tool):  python tools/wgrad_probe.py 64 144 133 8 32 56 56 [stride]

kind 133 = (1,3,3) pad (0,1,1), stride (1,s,s); 311 = (3,1,1) pad (1,0,0), stride (s,1,1).  Prints the instance the library picks and the
median of 5 samples of 200 launches."""
import ctypes, json, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from protoasnet_amd import _lib
from protoasnet_amd._lib import ConvDesc

cin, cout, kind, n, t, h, w = [int(v) for v in sys.argv[1:8]]
stride = int(sys.argv[8]) if len(sys.argv) > 8 else 1
k, p, s = ((1, 3, 3), (0, 1, 1), (1, stride, stride)) if kind == 133 else ((3, 1, 1), (1, 0, 0), (stride, 1, 1))
rup = lambda v, m: (v + m - 1) // m * m
to, ho, wo = [(i + 2 * p[j] - k[j]) // s[j] + 1 for j, i in enumerate((t, h, w))]
d = ConvDesc(N=n, Ti=t, Hi=h, Wi=w, Cin=cin, Cin_p=rup(cin, 8), To=to, Ho=ho, Wo=wo, Cout=cout, Cout_p=rup(cout, 8), kt=k[0], kh=k[1], kw=k[2],
             st=s[0], sh=s[1], sw=s[2], pt=p[0], ph=p[1], pw=p[2])
lib = _lib.lib()
dev = torch.device("cuda")
x = torch.randn(n, t, h, w, d.Cin_p, device=dev).bfloat16()
dy = torch.randn(n, to, ho, wo, d.Cout_p, device=dev).bfloat16()
taps = k[0] * k[1] * k[2]
dw = torch.zeros(cout, cin, taps, device=dev)
nb = int(lib.pasn_conv3d_wgrad_workspace_bytes(ctypes.byref(d), 1))
ws = torch.empty(max(nb, 4) // 4, device=dev)
st = torch.cuda.current_stream().cuda_stream
def run():
    _lib.check(lib.pasn_conv3d_wgrad_ws(x.data_ptr(), dy.data_ptr(), dw.data_ptr(), ctypes.byref(d), 1, ws.data_ptr() if nb else 0, st))
for _ in range(3): run()
torch.cuda.synchronize()
samples = []
for _ in range(5):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(200): run()
    e1.record(); torch.cuda.synchronize()
    samples.append(round(e0.elapsed_time(e1) * 5, 2))
variant = lib.pasn_conv3d_wgrad_variant(ctypes.byref(d), 1, 1 if nb else 0)
print(f"wgrad {cin}->{cout} k{kind} s{stride} {n}x{t}x{h}x{w}: {statistics.median(samples):.1f} us  variant {variant}  ws {nb / 1e6:.1f} MB  env={ {k_: v for k_, v in os.environ.items() if k_.startswith('PASN_')} }")
print(json.dumps({"wgrad_probe": f"{cin}->{cout} k{kind} s{stride} {n}x{t}x{h}x{w}", "variant": variant, "samples_us": samples, "median_us": statistics.median(samples)}))
