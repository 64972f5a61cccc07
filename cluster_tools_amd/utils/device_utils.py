"""What the GPU job scripts share: the device context on CC_DEVICE and the uint64 label I/O.
torch and _lib are imported inside the functions (job scripts import this module at start)."""
import os
from contextlib import contextmanager

import numpy as np

import cluster_tools_amd.utils.volume_utils as vu


@contextmanager
def job_context(torch_stream=False):
    """`with job_context() as (ctx, dev)`: the _lib.Context of this job's GPU (environment CC_DEVICE,
    default 0) and its torch device.  torch_stream=True makes that GPU torch's current device and
    runs the context on torch's current stream."""
    import torch
    from cluster_tools_amd import _lib
    device = int(os.environ.get('CC_DEVICE', '0'))
    dev = torch.device('cuda', device)
    if torch_stream:
        torch.cuda.set_device(dev)
    with _lib.Context(device) as ctx:
        if torch_stream:
            ctx.set_stream(torch.cuda.current_stream(dev).cuda_stream)
        yield ctx, dev


def read_labels_u64(path, key):
    """The whole label dataset as a contiguous uint64 array."""
    with vu.file_reader(path, 'r') as f:
        a = f[key][:]
    if a.dtype.kind not in 'ui':
        raise ValueError('%s/%s: integer labels expected, got %s' % (path, key, a.dtype))
    return np.ascontiguousarray(a.astype(np.uint64, copy=False))


def labels_to_device(a, dev):
    """uint64 labels on the device, as the int64 tensor of the same bits."""
    import torch
    return torch.from_numpy(a.view(np.int64)).to(dev)
