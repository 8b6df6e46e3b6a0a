"""Timing helpers shared by the bench_*.py tools of the fp32 4-D stage."""
import torch


def timed(fn, iters):
    """Median of ``iters`` HIP-event timings of ``fn()`` in ms, after one warm-up call."""
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        torch.cuda.synchronize()
        ts.append(s.elapsed_time(e))
    ts.sort()
    return ts[len(ts) // 2]


def peak_mib(fn):
    """Peak device memory of ``fn()`` above what is allocated before it, in MiB."""
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20
