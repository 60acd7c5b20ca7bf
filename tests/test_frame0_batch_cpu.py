"""The batched frame-0 op without a GPU: torch.ops.velocity_hip.frame0_init is registered when libvelocity_torch.so loads, and CPU frames are refused
(there is no CPU kernel)."""
import numpy as np
import pytest
import torch


def test_frame0_init_op_is_registered_and_refuses_cpu_frames():
    import velocity_amd.torch_ops  # noqa: F401
    from velocity_amd import _lib

    assert _lib.load().vh_version() >= 106
    op = torch.ops.velocity_hip.frame0_init
    assert "max_corners" in str(op.default._schema)
    frames = torch.zeros((2, 64, 64), dtype=torch.uint8)
    q = torch.from_numpy(np.tile(np.float32([[20, 20], [40, 20], [40, 30], [20, 30]]), (2, 1, 1)))
    with pytest.raises((RuntimeError, NotImplementedError)):
        op(frames, q, torch.eye(3, dtype=torch.float64), torch.zeros((4, 3), dtype=torch.float64), 10, 10)
