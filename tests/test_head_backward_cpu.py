"""The torch side of the head backward (vidil_amd/losses.py) without a GPU: the exact three-plane split of the upstream gradient
and the normalize / cross-entropy backward formulas against fp64 autograd."""
import pytest
import torch

from vidil_amd import losses as L


def _planes_exact(v, dtype, dim):
    hi, mid, lo, inv = L.split3_planes(v, dtype, dim)
    assert hi.dtype == mid.dtype == lo.dtype == dtype and inv.dtype == torch.float32
    rec = (hi.double() + mid.double() + lo.double()) * inv.double()
    assert torch.equal(rec, v.double()), (rec - v.double()).abs().max().item()
    # the scale is a power of two that puts every non-zero slice's largest magnitude into [2^10, 2^11]
    m, _ = torch.frexp(inv)
    assert torch.all(m == 0.5)
    top = (v.abs() / inv).amax(dim=dim)
    nz = v.abs().amax(dim=dim) > 0
    assert torch.all((top[nz] >= 1024) & (top[nz] < 2048))
    assert torch.all(hi[(v == 0)] == 0)


@pytest.mark.parametrize("dim", [0, 1])
def test_three_planes_reconstruct_bf16(dim):
    """bf16: 3 x 8 bits hold every f32, whatever the range inside a slice."""
    g = torch.Generator().manual_seed(0)
    v = torch.randn(33, 256, generator=g) * 1e-5
    v[3] = 0
    v[:, 7] = 0
    v[5] *= 1e-2                       # a row at 1e-7
    v[9, :8] = torch.tensor([1e-7, -1e-7, 3e-3, 1e-30, 0.0, 2.0 ** -100, 1.0, -1e-12])
    _planes_exact(v, torch.bfloat16, dim)


@pytest.mark.parametrize("dim", [0, 1])
def test_three_planes_reconstruct_f16_with_the_scale(dim):
    """f16: exact for elements of at least 2^-12 of their slice's largest — gradients at 1e-7 and 1e-3 in SEPARATE slices of
    the scaled axis, rows of zeros; without the scale every one of these values would be an f16 subnormal or zero."""
    g = torch.Generator().manual_seed(1)
    mag = torch.empty(40, 64).uniform_(1.0, 1000.0, generator=g) * torch.where(torch.rand(40, 64, generator=g) < 0.5, -1.0, 1.0)
    scale = torch.tensor([1e-7, 1e-3, 1e-5, 1.0])[torch.arange(40 if dim == 1 else 64) % 4]
    v = mag * (scale[:, None] if dim == 1 else scale[None, :]) * 1e-3
    if dim == 1:
        v[4] = 0
    else:
        v[:, 4] = 0
    assert v[v != 0].abs().min() < 1e-9 and (v[v != 0].abs() < 6e-8).any()
    _planes_exact(v, torch.float16, dim)


def test_normalize_backward_against_fp64_autograd():
    g = torch.Generator().manual_seed(2)
    p = torch.randn(6, 256, generator=g, dtype=torch.float64).requires_grad_(True)
    up = torch.randn(6, 256, generator=g, dtype=torch.float64)
    (torch.nn.functional.normalize(p, dim=-1) * up).sum().backward()
    got = L.normalize_backward(up, p.detach())
    assert torch.allclose(got, p.grad, rtol=1e-12, atol=1e-14)
    # mean over frames, then normalise: every frame's row receives 1/N of its sample's gradient
    q = torch.randn(6, 3, 256, generator=g, dtype=torch.float64).requires_grad_(True)
    (torch.nn.functional.normalize(q.mean(1), dim=-1) * up).sum().backward()
    got = (L.normalize_backward(up, q.detach().mean(1)) / 3)[:, None].expand(6, 3, 256)
    assert torch.allclose(got, q.grad, rtol=1e-12, atol=1e-14)


def test_cross_entropy_backward_against_fp64_autograd():
    g = torch.Generator().manual_seed(3)
    z = torch.randn(18, 2, generator=g, dtype=torch.float64).requires_grad_(True)
    labels = torch.cat([torch.ones(6, dtype=torch.long), torch.zeros(12, dtype=torch.long)])
    torch.nn.functional.cross_entropy(z, labels).backward()
    assert torch.allclose(L.cross_entropy_backward(z.detach(), labels), z.grad, rtol=1e-12, atol=1e-15)


def test_linear_backward_refuses_bad_shapes_before_any_launch():
    from vidil_amd.kernels import VidilHipError
    bf = torch.bfloat16
    with pytest.raises(VidilHipError):
        L.linear_backward(torch.zeros(4, 8), torch.zeros(5, 64, dtype=bf), torch.zeros(8, 64, dtype=bf))
    with pytest.raises(VidilHipError):
        L.linear_backward(torch.zeros(4, 8, dtype=bf), torch.zeros(4, 64, dtype=bf), torch.zeros(8, 64, dtype=bf))
    with pytest.raises(VidilHipError):
        L.linear_backward(torch.zeros(4, 8), torch.zeros(4, 64, dtype=torch.float16), torch.zeros(8, 64, dtype=bf))
    with pytest.raises(VidilHipError, match="CUDA/HIP"):        # good shapes: no CPU fallback
        L.linear_backward(torch.zeros(4, 8), torch.zeros(4, 64, dtype=bf), torch.zeros(8, 64, dtype=bf))


def test_the_four_loss_forwards_carry_head_grads():
    import inspect

    from vidil_amd.blip_pretrain import BLIP_Pretrain, BLIP_Pretrain_Video
    from vidil_amd.blip_retrieval import BLIP_Retrieval, BLIP_Retrieval_Video

    for cls in (BLIP_Retrieval, BLIP_Retrieval_Video, BLIP_Pretrain, BLIP_Pretrain_Video):
        par = inspect.signature(cls.forward).parameters
        assert par["head_grads"].kind is inspect.Parameter.KEYWORD_ONLY and par["head_grads"].default is None, cls.__name__
        assert par["grads"].kind is inspect.Parameter.KEYWORD_ONLY, cls.__name__
    assert inspect.signature(BLIP_Retrieval.loss_forward).parameters["head_grads"].default is None
