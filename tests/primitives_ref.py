"""Float64 references and gates of the CSR segment primitives (csrc/segment.hip) and of the weighted row BatchNorm
(csrc/rowbn.hip).  Plain Python, imported by name like ``tolerances.py`` and ``rowwise.py``.

The references are written from the reference project's expressions (torch_scatter's CSR semantics, pooling.py:758-856,
``nn.BatchNorm1d`` over the gathered views), not from the kernels.  Every function takes ``dtype``: ``torch.float64`` is
the reference, ``torch.float32`` the plain torch fp32 evaluation of the same case whose own error may raise a gate
(``tolerances.gate``).  Inputs are always the *stored* data (a bf16 / fp16 tensor is cast up exactly).

Gates (none typed in here):

* fp32 storage: ``tolerances.rel_err`` against float64, held to ``tolerances.gate(cls, fp32_err)``.
* bf16 / fp16 storage: the kernels accumulate in fp32 and round once on store, so elementwise
  ``|got - ref64| <= 0.5 * ulp(ref64, dtype) + g * max|ref64|`` with ``g`` the fp32 gate of the same tensor.  One
  round-to-nearest-even meets it; a truncating store (up to 1 ulp) or a second rounding does not.
  ``tests/test_primitives_ref_host.py`` shows the bound is attained to 0.97 .. 1.0 by a correct fp32 emulation.
* exact quantities (max / min values, every arg, gathers, max / min gradients given the arg): ``torch.equal``.
"""
import torch
import torch.nn.functional as F

import tolerances as T
from oracle import pooling_oracle as O

MANT_BITS = {torch.bfloat16: 7, torch.float16: 10}     # stored fraction bits
MIN_EXP = {torch.bfloat16: -126, torch.float16: -14}   # exponent of the smallest normal: below it the spacing is fixed


# ----------------------------------------------------------------------------------------------
# CSR helpers
# ----------------------------------------------------------------------------------------------
def dense_index(ptr):
    return O.dense_index(ptr)


def group_sizes(ptr):
    return ptr[1:] - ptr[:-1]


def segment_arg(src, ptr, reduce):
    """First row attaining the extremum, -1 for empty groups (``oracle.pooling_oracle.segment_arg``, vectorised form:
    the host tests hold the two against each other)."""
    return O.segment_arg_fast(src, ptr, reduce)


def segment_ref(src, ptr, reduce, dtype=torch.float64):
    """torch_scatter.segment_csr along dim 0 -> (out, arg); empty groups give 0, ``arg`` is None for sum / mean."""
    x = src.detach().to(dtype)
    n = ptr.shape[0] - 1
    if reduce in ("sum", "mean"):
        out = torch.zeros((n, x.shape[1]), dtype=dtype).index_add_(0, dense_index(ptr), x)
        if reduce == "mean":
            out = out / group_sizes(ptr).clamp(min=1).to(dtype).view(-1, 1)
        return out, None
    arg = segment_arg(x, ptr, reduce)
    x0 = torch.cat([x, torch.zeros((1, x.shape[1]), dtype=dtype)])
    return x0.gather(0, torch.where(arg < 0, torch.full_like(arg, x.shape[0]), arg)), arg


def segment_grad_ref(gout, ptr, reduce, arg, n_rows, dtype=torch.float64):
    """Gradient of ``segment_ref`` w.r.t. its source: sum copies, mean divides by the group size, max / min route the
    group's gradient to the arg row only."""
    g = gout.detach().to(dtype)
    idx = dense_index(ptr)
    if reduce == "sum":
        return g[idx]
    if reduce == "mean":
        return (g / group_sizes(ptr).clamp(min=1).to(dtype).view(-1, 1))[idx]
    out = torch.zeros((n_rows + 1, g.shape[1]), dtype=dtype)
    out.scatter_(0, torch.where(arg < 0, torch.full_like(arg, n_rows), arg), g)
    return out[:n_rows]


def gather_ref(src, ptr):
    """pooling.py:813-841, any dtype, exact."""
    return src[dense_index(ptr)]


def softmax_ref(src, ptr, eps=1e-12, scaling=False, gout=None, dtype=torch.float64):
    """pooling.py:758-810 (``oracle.pooling_oracle.segment_softmax_csr``; the group size's square root in ``dtype``
    too): centre on the group max, divide by sqrt(size) after centring, exp, divide by (group sum + eps).
    Returns (out, grad) with ``grad`` the gradient of ``(out * gout).sum()`` (None without ``gout``).  As in the
    reference, the group max is part of the graph (pooling.py:787 differentiates through ``segment_csr(.., 'max')``):
    with ``eps`` the outputs of a group do not sum to one, and the arg row of the max receives
    ``-sum_i(gout_i out_i) eps / ((S + eps) d)`` on top of the usual softmax gradient."""
    x = src.detach().to(dtype).requires_grad_()
    idx = dense_index(ptr)
    arg = segment_arg(x, ptr, "max")
    x0 = torch.cat([x, torch.zeros((1, x.shape[1]), dtype=dtype)])
    mx = x0.gather(0, torch.where(arg < 0, torch.full_like(arg, x.shape[0]), arg))
    centered = x - mx[idx]
    if scaling:
        centered = centered / group_sizes(ptr).to(dtype).sqrt()[idx].view(-1, 1)
    e = centered.exp()
    den = torch.zeros((ptr.shape[0] - 1, x.shape[1]), dtype=dtype).index_add(0, idx, e)
    out = e / (den + eps)[idx]
    grad = None
    if gout is not None:
        (grad,) = torch.autograd.grad((out * gout.to(dtype)).sum(), x)
    return out.detach(), grad


# ----------------------------------------------------------------------------------------------
# weighted BatchNorm + LeakyReLU on rows
# ----------------------------------------------------------------------------------------------


def view_index(R, counts):
    cnt = torch.ones(R, dtype=torch.long) if counts is None else counts.long().cpu()
    return torch.repeat_interleave(torch.arange(R), cnt), cnt


def rowbn_ref(y, counts, gamma, beta, slope, gview=None, running=None, eps=1e-5, side=None, out_got=None, z32=None,
              dtype=torch.float64):
    """``leaky_slope(nn.BatchNorm1d(y[idx]))`` with ``idx = repeat_interleave(arange(R), counts)`` (the gathered views;
    every row once when ``counts`` is None), batch statistics unless ``running = (mean, var)`` is given (eval mode).

    Returns a dict: ``out`` [R, C] (the module's own output at the first view of every seen row; rows without views are
    normalised with the same batch statistics), ``z`` (pre-activation, all rows), ``mean`` / ``var`` (biased) / ``n`` of
    the views, and with ``gview`` [R, C] (the loss is ``sum_v out_v * gview[idx_v]``) ``dy`` / ``dgamma`` / ``dbeta``.

    ``side`` [R, C] bool: which side of the kink every element is differentiated on (True = z > 0).  The derivative of
    LeakyReLU is discontinuous at z = 0, and an element whose |z| is within the fp32 error of z may legitimately fall
    on either side; a caller passes the float64 side with those elements taken from the run under test, so that one such
    element cannot move dgamma / dbeta by a whole term.  ``out_got`` (the output of the run under test) and ``z32``
    (the pre-activation of the plain fp32 evaluation of the same case) make ``kink_side`` build that mask: the window
    is FP32_HEADROOM x max|z32 - z64|, measured, not typed in.  The mask comes back as ``side`` for the fp32 twin,
    the number of elements inside the window as ``n_kink``.  None = ``F.leaky_relu``'s own derivative."""
    R, C = y.shape
    idx, cnt = view_index(R, counts)
    y_ = y.detach().cpu().to(dtype).requires_grad_()
    bn = torch.nn.BatchNorm1d(C, eps=eps, affine=gamma is not None).to(dtype)
    if gamma is not None:
        with torch.no_grad():
            bn.weight.copy_(gamma.detach().cpu().to(dtype))
            bn.bias.copy_(beta.detach().cpu().to(dtype))
    yv = y_[idx]
    if running is None:
        bn.train()
        mean, var = yv.detach().mean(0), yv.detach().var(0, unbiased=False)
    else:
        bn.eval()
        mean, var = running[0].detach().cpu().to(dtype), running[1].detach().cpu().to(dtype)
        bn.running_mean.copy_(mean)
        bn.running_var.copy_(var)
    zv = bn(yv)
    with torch.no_grad():
        z = F.batch_norm(y_.detach(), mean.clone(), var.clone(), bn.weight, bn.bias, False, 0.0, eps)
        first = (cnt.cumsum(0) - cnt)[cnt > 0]
        z[cnt > 0] = zv.detach()[first]                 # seen rows: the module's own numbers
    n_kink = 0
    if side is None and out_got is not None:
        side, n_kink = kink_side(z.double(), out_got, z32)
    res = dict(out=F.leaky_relu(z, slope), z=z, mean=mean, var=var, n=float(cnt.sum()), side=side, n_kink=n_kink)
    if gview is not None:
        if side is None:
            ov = F.leaky_relu(zv, slope)
        else:
            one = torch.ones((), dtype=dtype)
            ov = zv * torch.where(side.cpu(), one, one * float(slope))[idx]
        params = [bn.weight, bn.bias] if gamma is not None else []
        grads = torch.autograd.grad((ov * gview.detach().cpu().to(dtype)[idx]).sum(), [y_] + params)
        res["dy"] = grads[0]
        if params:
            res["dgamma"], res["dbeta"] = grads[1], grads[2]
    return res


def kink_side(z64, out_got, z32):
    """(The float64 side of the kink, with the elements whose |z64| is within FP32_HEADROOM x the measured fp32 error
    of z taken from the run under test; the number of such elements)."""
    window = T.FP32_HEADROOM * float((z32.detach().double() - z64).abs().max())
    near = z64.abs() <= window
    return torch.where(near, out_got.detach().cpu().double() > 0, z64 > 0), int(near.sum())


# ----------------------------------------------------------------------------------------------
# gates
# ----------------------------------------------------------------------------------------------
def ulp(ref64, dtype):
    """Spacing of ``dtype`` (bf16 / fp16) at |ref64|; below the smallest normal the (subnormal) spacing is constant."""
    _, e = torch.frexp(ref64.detach().double().abs())          # |x| = m 2^e, m in [0.5, 1)
    e = (e - 1).clamp(min=MIN_EXP[dtype])                       # zero: frexp gives e = 0, far below -> clamped as well
    e = torch.where(ref64 == 0, torch.full_like(e, MIN_EXP[dtype]), e)
    return torch.ldexp(torch.ones_like(ref64, dtype=torch.float64), e - MANT_BITS[dtype])


def same_nonfinite(got, ref64):
    """Assert that ``got`` is +-inf exactly where the float64 reference is (same sign), and return both with those
    entries zeroed, for the finite comparison."""
    g, r = got.detach().cpu().double(), ref64.detach().cpu().double()
    bad = ~torch.isfinite(r)
    assert torch.equal(g[bad], r[bad]), "non-finite entries differ from the float64 reference"
    assert bool(torch.isfinite(g[~bad]).all()), "non-finite output where the float64 reference is finite"
    if bool(bad.any()):
        g, r = g.masked_fill(bad, 0.0), r.masked_fill(bad, 0.0)
    return g, r


def half_ulp_ratio(got, ref64, dtype, g, scale=None):
    """max over elements of |got - ref64| / (0.5 ulp(ref64, dtype) + g max|scale or ref64|): <= 1 meets the gate."""
    got, ref64 = same_nonfinite(got, ref64)
    if ref64.numel() == 0:
        return 0.0
    s = ref64 if scale is None else scale.detach().cpu().double()
    bound = 0.5 * ulp(ref64, dtype) + g * float(s.abs().max())
    return float(((got - ref64).abs() / bound).max())


class Report(T.Report):
    """``tolerances.Report`` with the storage-type rule: ``hold`` adds one row for a tensor against its float64
    reference -- the fp32 class gate for fp32 storage, the half-ulp rule (shown as err / bound against 1) otherwise."""

    def hold(self, case, name, cls, got, ref64, ref32, scale=None):
        r64 = ref64.detach().cpu().double()
        sc = None if scale is None else scale.detach().cpu().double()
        fin = torch.isfinite(r64)
        fp32_err = T.rel_err(torch.where(fin, ref32.detach().cpu().double(), r64).masked_fill(~fin, 0.0),
                             r64.masked_fill(~fin, 0.0), sc)
        if got.dtype == torch.float32:
            g, r = same_nonfinite(got, r64)
            return self.add(case, name, cls, T.rel_err(g, r, sc), fp32_err)
        ratio = half_ulp_ratio(got, r64, got.dtype, T.gate(cls, fp32_err), sc)
        self.rows.append((case, name, "half-ulp", ratio, 1.0, fp32_err))
        return ratio
