"""`skinny_linear_mfma` on CPU tensors (the torch expression) and what
`step_linear` does on the CPU; the kernel's tests and the batch-9..32 route
are in test_decode_gemv_mfma_gpu."""

import pytest
import torch

from tests import decode_gemv_oracles as go
from tests import kernel_oracles as ko


@pytest.mark.parametrize("fmt", ["fp8_e4m3", "bf16"])
@pytest.mark.parametrize("M", [9, 32])
def test_checker_passes_the_torch_implementation(fmt, M):
    from modalities_amd.ops import skinny_linear_mfma
    args = go.make_case(M, 33, 1040, fmt, True, seed=M, x_pad=32)
    ko.require(f"skinny_linear_mfma cpu {fmt} M{M}",
               go.check_skinny_linear(skinny_linear_mfma, *args))
    x, w, scale, bias = go.make_case(33, 8, 32, fmt, True, seed=5)
    with pytest.raises(ValueError, match="M must be"):
        skinny_linear_mfma(x, w, scale, bias)


def test_step_linear_routes_by_rows(monkeypatch):
    """The MFMA route is the device's (test_decode_gemv_mfma_gpu spies it at
    batch 12 and 20): on the CPU `step_linear` keeps what it did before, the
    torch expression up to 8 rows and F.linear above, whatever the switch
    says."""
    from modalities_amd.ops import decode_linear as dl
    lin = torch.nn.Linear(64, 24).to(torch.bfloat16)
    dl.set_prepared(lin, dl.prepare_linear(lin.weight, lin.bias, "fp8_e4m3"))
    calls = []
    for name in ("skinny_linear", "skinny_linear_mfma"):
        def spy(*a, _real=getattr(dl, name), _name=name, **k):
            calls.append(_name)
            return _real(*a, **k)
        monkeypatch.setattr(dl, name, spy)
    g = torch.Generator().manual_seed(0)
    x = torch.randn(33, 1, 64, generator=g).to(torch.bfloat16)
    for rows, want in ((8, ["skinny_linear"]), (9, []), (32, []), (33, [])):
        calls.clear()
        y = dl.step_linear(lin, x[:rows])
        assert calls == want and y.shape == (rows, 1, 24), rows
        if not want:
            assert torch.equal(y, lin(x[:rows]))
    assert dl.decode_mfma_min_rows() == 9
    dl.set_decode_mfma_min_rows(5)
    try:
        calls.clear()
        dl.step_linear(lin, x[:5])
        assert calls == ["skinny_linear"] and dl.decode_mfma_min_rows() == 5
        with pytest.raises(ValueError):
            dl.set_decode_mfma_min_rows(10)
    finally:
        dl.set_decode_mfma_min_rows(9)
