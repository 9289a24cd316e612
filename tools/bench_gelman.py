"""convergence_gelman's device reduction: [chains] x [p] columns x the second half of a [rows]-row history (default: config C4's
width, 512 x 50 x 10,000: 1.02 GB read per pass).  Two legs on the same tensor, alternating in one process:
  hip    fmcmc_gelman_partial_dev (any p <= 256): time (HIP events), window bytes per second, size of `work`;
  torch  the torch formulation of the same partial vector that convergence_gelman used above 64 columns until the HIP
         kernel covered them (kept here as the yardstick it was replaced against): time and peak torch memory.
Then the two partial vectors are compared, and the HIP leg is spot-checked against numpy on 8 chains."""
import ctypes as C, os, sys
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fmcmc_amd import _abi as abi
Cn = int(sys.argv[1]) if len(sys.argv) > 1 else 512
p = k = int(sys.argv[2]) if len(sys.argv) > 2 else 50
S = int(sys.argv[3]) if len(sys.argv) > 3 else 10000
REPS = int(sys.argv[4]) if len(sys.argv) > 4 else 5
row0, N = S // 2, S - S // 2
g = torch.Generator(device="cuda"); g.manual_seed(1)
x = torch.randn((Cn, k, S), dtype=torch.float64, device="cuda", generator=g) * 0.5 + 3.0
cols = torch.arange(p, dtype=torch.int32, device="cuda")
center = x[0, :, row0].contiguous()
L = abi.lib()
plen = int(L.fmcmc_gelman_partial_len(p))
part = torch.zeros(plen, dtype=torch.float64, device="cuda")
work = torch.empty(int(L.fmcmc_gelman_work_len(Cn, p)), dtype=torch.float64, device="cuda")
st = torch.cuda.current_stream().cuda_stream


def run_hip():
    rc = L.fmcmc_gelman_partial_dev(x.data_ptr(), Cn, k, S, row0, N, cols.data_ptr(), p, center.data_ptr(), work.data_ptr(),
                                    part.data_ptr(), C.c_void_p(st))
    assert rc == 0


def run_torch():
    """The partial with torch ops, in blocks of chains so that the gathered window, its centred copy and the products stay
    under three 256 MB temporaries (1024 chains x k = 100 x N = 5000 rows were three 4 GB tensors at once)."""
    partial = torch.zeros(plen, dtype=torch.float64, device="cuda")
    cols_l = cols.long()
    per_chain = 3 * p * N * 8
    blk_c = max(1, min(Cn, (256 << 20) // max(per_chain, 1)))
    xbm = torch.empty((Cn, p), dtype=torch.float64, device="cuda")
    s2 = torch.empty((Cn, p), dtype=torch.float64, device="cuda")
    sum_xx = torch.zeros((p, p), dtype=torch.float64, device="cuda")
    sum_S = torch.zeros((p, p), dtype=torch.float64, device="cuda")
    for c0 in range(0, Cn, blk_c):
        X = x[c0:c0 + blk_c][:, cols_l, row0:row0 + N] - center[None, :, None]
        xb_b = X.mean(dim=2)
        X -= xb_b[:, :, None]
        Sc = X @ X.transpose(1, 2) / float(N - 1)
        xbm[c0:c0 + blk_c] = xb_b
        s2[c0:c0 + blk_c] = Sc.diagonal(dim1=1, dim2=2)
        sum_xx += (xb_b[:, :, None] * xb_b[:, None, :]).sum(0)
        sum_S += Sc.sum(0)
        del X, Sc
    partial[0] = float(Cn)
    o = 1
    for blk in (xbm.sum(0), sum_xx.reshape(-1), sum_S.reshape(-1), s2.sum(0), (s2 * s2).sum(0),
                (s2 * xbm).sum(0), (s2 * xbm * xbm).sum(0)):
        partial[o:o + blk.numel()] = blk
        o += blk.numel()
    return partial


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); out = fn(); e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


run_hip(); part_t = run_torch(); torch.cuda.synchronize()          # warm both legs at this shape
base = torch.cuda.memory_allocated()
torch.cuda.reset_peak_memory_stats()
t_hip, t_torch = [], []
for _ in range(REPS):                                               # alternating, same process
    t_hip.append(timed(run_hip)[0])
    ms, part_t = timed(run_torch)
    t_torch.append(ms)
peak = torch.cuda.max_memory_allocated() - base
byt = Cn * p * N * 8
ms = min(t_hip)
print("gelman partial: %d chains x p=%d x N=%d rows (%.2f GB window): %.3f ms, %.0f GB/s of window bytes, %.1f GFLOP/s (syrk)" % (
    Cn, p, N, byt / 1e9, ms, byt / ms / 1e6, Cn * p * p * N * 2 / ms / 1e6))
print("  hip   leg: min %.3f ms, median %.3f ms of %d; work %.1f MB" % (ms, float(np.median(t_hip)), REPS, work.numel() * 8 / 1e6))
print("  torch leg: min %.3f ms, median %.3f ms of %d; peak torch memory above the inputs %.1f MB" % (
    min(t_torch), float(np.median(t_torch)), REPS, peak / 1e6))
ph, pt = part.cpu().numpy(), part_t.cpu().numpy()
print("  partial, hip against torch: max |diff| / max|.| %.2e" % (np.abs(ph - pt).max() / np.abs(pt).max()))
# spot check against numpy on 8 chains
nc = min(Cn, 8)
w = x[:nc, :, row0:].cpu().numpy().transpose(0, 2, 1)
xb = w.mean(1) - center.cpu().numpy()
wk = work.cpu().numpy().reshape(Cn, p + p * p)
print("max |xbar err| %.2e, max rel |S_c err| %.2e" % (np.abs(wk[:nc, :p] - xb).max(),
      max(np.abs(wk[c, p:].reshape(p, p) - np.cov(w[c].T, ddof=1)).max() / np.abs(np.cov(w[c].T, ddof=1)).max() for c in range(nc))))
