"""What the wrappers of the volume operations (prep.py, postprocess.py, preprocess.py) share: the Python half of the workspace
contract of csrc/volume.h (query -> allocate -> call -> read a one-int status) and the numpy / tensor conversion of a mask.
Allocations go through ``torch.empty`` looked up at call time, like everywhere else in the package."""
import numpy as np
import torch

from . import _lib


def workspace(query, *extents, device, what=None, min_bytes=0):
    """The uint8 workspace tensor a ``seunet_*_workspace_bytes`` query asks for.  ``what`` (the caller's "<module prefix>:
    <function>"): a 0-byte answer (rejected extents) raises ValueError with the library's message behind it; without it the
    answer is taken as it is, at least ``min_bytes``."""
    nbytes = int(query(*extents))
    if nbytes == 0 and what is not None:
        raise ValueError(f"{what}: {_lib.last_error()}")
    return torch.empty(max(nbytes, min_bytes), dtype=torch.uint8, device=device)


def read_status(status) -> int:
    """The one-int status a launcher left on the device (synchronises)."""
    return int(status.item())


def upload_mask(a: np.ndarray):
    """numpy array of any dtype (non-zero = 1) -> uint8 CUDA tensor of zeros and ones."""
    return torch.from_numpy(np.ascontiguousarray(a != 0).view(np.uint8)).cuda()


def mask_in(a, name, prefix, tensor_in):
    """A 0/1 volume argument -> (uint8 CUDA tensor, came-as-numpy).  A 3-D numpy array is uploaded; anything else goes through
    the caller's ``tensor_in(a, name)``, which holds its dtype policy."""
    if isinstance(a, np.ndarray):
        if a.ndim != 3:
            raise ValueError(f"{prefix}: `{name}` must be (n0, n1, n2), got {tuple(a.shape)}")
        if not torch.cuda.is_available():
            raise RuntimeError(f"{prefix}: `{name}` needs a GPU (there is no CPU path)")
        return upload_mask(a), True
    return tensor_in(a, name), False


def out(t, as_numpy):
    """numpy in -> numpy out, CUDA tensor in -> CUDA tensor out."""
    return t.cpu().numpy() if as_numpy else t
