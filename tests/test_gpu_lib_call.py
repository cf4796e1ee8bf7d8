"""-m gpu: _lib.call on a real launch -- the arguments arrive in order and the launch goes to torch's current stream (or the one given)."""
import pytest
import torch

import mapfree_reloc_amd as mfr

pytestmark = pytest.mark.gpu
_lib = mfr._lib


def test_call_launches_on_the_current_stream_and_on_the_given_one():
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(7)
    x0 = torch.randn(1, 4, 4, 4, generator=g).to(dev)
    bias = torch.randn(4, generator=g).to(dev)
    want = torch.relu(x0 + bias[None, :, None, None])
    assert bool((want == 0).any()) and bool((want > 0).any())                      # both sides of the ReLU occur
    torch.cuda.synchronize(dev)

    side = torch.cuda.Stream(dev)
    x = x0.clone()
    torch.cuda.synchronize(dev)
    with torch.cuda.stream(side):
        assert _lib.stream_ptr() == side.cuda_stream
        _lib.call("mfr_bias_relu_nchw", x, bias, 1, 4, 16)
    side.synchronize()
    assert torch.equal(x, want)

    y = x0.clone()
    torch.cuda.synchronize(dev)
    _lib.call("mfr_bias_relu_nchw", y, bias, 1, 4, 16, stream=None)                # the null stream, explicitly
    torch.cuda.synchronize(dev)
    assert torch.equal(y, want) and torch.equal(y, x)
