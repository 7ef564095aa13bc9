"""What every call into libspadot_model.so shares: device pointers, the current stream, and the reading of a return code."""
import ctypes

import torch


def ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def need_cuda(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise RuntimeError("spadot_amd ops run on the MI355X only (got a CPU tensor); there is no CPU path")


def launched(rc, name, limits=None, detail=""):
    """Reads the return code of entry `name`: -7 of an entry with stated limits is a ValueError (detail: what the call held),
    any other non-zero code a RuntimeError."""
    if rc == -7 and limits is not None:
        raise ValueError(f"{name}: outside its limits ({limits}){detail}")
    if rc != 0:
        raise RuntimeError(f"{name} failed with {rc}")
