"""Diagnostic: the phases of the folded tail (gemm_mfma.h, MODE 4) at the headline shape.  Needs a stamps build of the
library (`make -C torch-geometric-pool_amd/csrc stamps`, or tools/build_gemm_variant.sh NAME -DTGP_GEMM_STAMPS):

  python tools/fold_tail_stamps.py [LIB [B N K F [p]]]      default: lib/libtgp_hip_stamps.so, C2 (32 1024 128 64, p = 0.01
                                                             before symmetrising: ~2 % nonzeros)

Thread 0 of every workgroup stamps the 100 MHz clock at kernel entry (slot 0), at the end of the k-loop (2), before the
tail's first MFMA (8), at three points of the tail (9, 10, 11) and at the end (3):

  slot   two-phase tail (TGP_FOLD_SPLIT = 1)              one-phase tail (TGP_FOLD_SPLIT = 0)
  9      S^T U multiplied                                  all 192 MFMAs issued
  10     S^T U parked in LDS (12 k-groups of S^T X done)   P in LDS
  11     S^T X multiplied, S^T U stored                    column sums written

With block-order slabs (TGP_FOLD_BLOCKS = 1, the shipped form) nothing is parked: slot 10 is the same point of the X-part
(12 of its 32 k-groups done, the four S^T U block stores issued behind the first four) and slot 11 its end.

Without the X-part (TGP_FOLD_X_LATE = 1, the shipped form: S^T X is formed by post_rows_kernel<true>) slot 9 is the end
of the tail's MFMAs, slot 10 the four S^T U block stores issued, slot 11 the column-sum partials added lane to lane, and
the end follows the partials' one barrier and the ordered add.

The stamps slow the launch, so the figures are shares; median and p10..p90 over the workgroups, in us."""
import ctypes
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
lib_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "torch-geometric-pool_amd", "lib", "libtgp_hip_stamps.so")
os.environ["TGP_HIP_LIB"] = os.path.abspath(lib_path)
sys.path.insert(0, os.path.join(ROOT, "torch-geometric-pool_amd"))

import torch  # noqa: E402
from tgp import _native, kernels  # noqa: E402

B, N, K, F = (int(v) for v in sys.argv[2:6]) if len(sys.argv) > 5 else (32, 1024, 128, 64)
p = float(sys.argv[6]) if len(sys.argv) > 6 else 0.01
dev = torch.device("cuda:0")
g = torch.Generator(device=dev).manual_seed(0)
A = (torch.rand(B, N, N, device=dev, generator=g) < p).float()
A = torch.maximum(A, A.transpose(1, 2)).contiguous()
A.diagonal(dim1=1, dim2=2).zero_()
X = torch.randn(B, N, F, device=dev, generator=g)
S = torch.softmax(torch.randn(B, N, K, device=dev, generator=g), -1)
flags = kernels.dense_flags(True, True, True, False)

lib = _native.lib()
lib.tgp_debug_set_gemm_stamps.argtypes = [ctypes.c_void_p]
for _ in range(3):
    kernels.dense_pool(S, A, X, flags)
nwg = B * ((N + 127) // 128)
stamps = torch.zeros(nwg * 16, dtype=torch.int64, device=dev)
assert lib.tgp_debug_set_gemm_stamps(stamps.data_ptr()) == 0
torch.cuda.synchronize()
kernels.dense_pool(S, A, X, flags)
torch.cuda.synchronize()
assert lib.tgp_debug_set_gemm_stamps(None) == 0
st = stamps.view(-1, 16).cpu()
st = st[st[:, 0] > 0]
assert st.size(0) == nwg and (st[:, 8] > 0).all(), "the call did not take the folded route"
us = lambda a, b: (st[:, b] - st[:, a]).double() / 100.0  # noqa: E731


def q(v):
    v = v.sort()[0]
    n = v.numel()
    return f"{float(v[n // 2]):6.2f}  ({float(v[int(0.1 * (n - 1))]):.2f}..{float(v[int(0.9 * (n - 1))]):.2f})"


print(f"{os.path.basename(lib_path)}: {nwg} workgroups, launch span {float((st[:, 3].max() - st[:, 0].min())) / 100.0:.2f} us")
for name, a, b in (("entry -> k-loop end", 0, 2), ("k-loop end -> first MFMA", 2, 8), ("slot 8 -> 9", 8, 9), ("slot 9 -> 10", 9, 10),
                   ("slot 10 -> 11", 10, 11), ("slot 11 -> end", 11, 3), ("tail: k-loop end -> end", 2, 3)):
    print(f"{name:30s} {q(us(a, b))}")
