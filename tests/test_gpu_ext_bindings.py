"""Every binding of the HIP extension rejects, with a Python exception and
before anything is launched, a tensor argument that is on the CPU, on another
device, or of the wrong dtype. Extends test_moe_gemm_w4_argument_checks to
all ops and all tensor arguments (cases: binding_cases.py)."""
import pytest
import torch

import binding_cases as bc
from bloombee_amd import ops

DEV = "cuda:0"
_DTYPE = r"must be (bf16|f16|f32|int32|u8|bool)"


def _snapshot(call):
    return {i: call.args[i].clone() for i in call.inplace}


@pytest.mark.gpu
@pytest.mark.parametrize("op", bc.OPS)
def test_argument_checks(op):
    call = bc.build(DEV)[op]
    f = getattr(ops.hip_ops, op)
    f(*call.args)                          # the arguments are valid
    torch.cuda.synchronize()
    before = _snapshot(call)
    for i in call.tensor_args():           # every tensor argument, in turn
        bad = list(call.args)
        bad[i] = bad[i].cpu()
        with pytest.raises(RuntimeError, match="must be on device"):
            f(*bad)
    i, dtype = call.bad_dtype
    bad = list(call.args)
    bad[i] = bad[i].to(dtype)
    with pytest.raises(RuntimeError, match=_DTYPE):
        f(*bad)
    torch.cuda.synchronize()
    for i, want in before.items():         # rejected calls wrote nothing
        assert torch.equal(call.args[i], want), f"{op}: argument {i} changed"


@pytest.mark.gpu
def test_cross_device_rejected():
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two devices")
    for op, call in bc.build(DEV).items():
        f = getattr(ops.hip_ops, op)
        before = _snapshot(call)
        tensors = call.tensor_args()
        for i in tensors[1:]:
            bad = list(call.args)
            bad[i] = bad[i].to("cuda:1")
            with pytest.raises(RuntimeError, match="must be on the same device"):
                f(*bad)
        torch.cuda.synchronize()
        for i, want in before.items():
            assert torch.equal(call.args[i], want), f"{op}: argument {i} changed"
