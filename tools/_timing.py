"""What the tools/*_time.py scripts share: the device-event timing loop and the median / spread of a JSON record."""
import statistics


def median(v):
    return {"median_ms": round(statistics.median(v), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3)}


def timed(go, repeats, warm=True):
    """The device milliseconds of `repeats` calls of go(), each between two events; warm: one untimed call first."""
    import torch
    if warm:
        go()                                                                         # code object, allocator
        torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        go()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return ms
