"""hipGraph capture, as the trainers (step.py) and the evaluators (evaluate.py) do it."""
from __future__ import annotations

import contextlib

import torch

# hipGraph capture must not be invalidated by other threads' HIP calls: with an RCCL communicator alive, PyTorch's
# watchdog thread polls events while the step is being captured ("global" mode would then abort the capture).
_CAPTURE_MODE = "thread_local"


def graph(g: torch.cuda.CUDAGraph, pool=None):
    """``torch.cuda.graph(g)`` in the capture mode of this package, in ``pool`` if one is given."""
    return torch.cuda.graph(g, pool=pool, capture_error_mode=_CAPTURE_MODE)


@contextlib.contextmanager
def warmup_stream(device):
    """The eager warm-up in front of a capture: the body runs on a side stream of ``device`` that has waited for the current
    stream; afterwards the current stream waits for the side stream and the host for the device."""
    main = torch.cuda.current_stream()
    side = torch.cuda.Stream(device=device)
    side.wait_stream(main)
    with torch.cuda.stream(side):
        yield
    main.wait_stream(side)
    torch.cuda.synchronize()
