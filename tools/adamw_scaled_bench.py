"""`usc_adamw_step_scaled` alone, HBM-cold, next to `flat.div_(world)` + `usc_adamw_step`: µs per call, bytes moved and
the fraction of the achievable HBM bandwidth (6.29 TB/s, tools/hbm_report.py) on the model's 39.6 M parameters.  Two
buffer sets of 4 x 158 MB alternate, so no call finds its operands in the 256 MB last-level cache."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from unscene3d_amd._lib import check, lib  # noqa: E402

ACHIEVABLE = 6.29e12
N = 39_600_000
dev = torch.device("cuda:0")
sets = [[torch.randn(N, device=dev) * 0.01 for _ in range(2)] + [torch.zeros(N, device=dev) for _ in range(2)]
        for _ in range(2)]
stream = torch.cuda.current_stream().cuda_stream
hp = (1e-4, 0.9, 0.999, 1e-8, 0.01)


def plain(k, i):
    p, g, m, v = sets[i]
    g.div_(2)
    check(lib.usc_adamw_step(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), N, *hp, k, stream), "usc_adamw_step")


def scaled(write_back):
    def fn(k, i):
        p, g, m, v = sets[i]
        check(lib.usc_adamw_step_scaled(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), N, 0.5, write_back, *hp, k,
                                        stream), "usc_adamw_step_scaled")
    return fn


def timed(fn, reps=20):
    for k in range(1, 4):
        fn(k, k % 2)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for k in range(4, 4 + reps):
        fn(k, k % 2)
    e1.record()
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / reps


print(f"parameters {N / 1e6:.1f} M; library: {lib.usc_build_info().decode()}")
for name, fn, bytes_per in (("div_ + usc_adamw_step", plain, 36), ("usc_adamw_step_scaled(write_back=0)", scaled(0), 28),
                            ("usc_adamw_step_scaled(write_back=1)", scaled(1), 32)):
    us = timed(fn)
    print(f"{name:38s} {us:8.1f} us  {bytes_per} B/param = {bytes_per * N / 1e6:7.1f} MB  "
          f"{bytes_per * N / (us * 1e-6) / 1e12:5.2f} TB/s = {bytes_per * N / (us * 1e-6) / ACHIEVABLE:4.0%} of achievable")
