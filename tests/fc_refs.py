"""Plain float64 / int64 statements of the FullyConnected entry points (rg_fc_forward, rg_fc_dgrad, rg_fc_wgrad,
rg_act_backward, rg_transpose_cast), the operands they are tested on and the derived error bounds.  torch on the CPU only;
tests/test_fc_kernel_statements.py holds reagent_amd/csrc/fc.hip and rg_gemm.h to them.

Bound of a GEMM element (any accumulation order, fused or not; Higham, Accuracy and Stability, 3.5, with one rounding per
product, one per addition, the bias addition and the output, gamma_n <= 2 n u here):
    |got - ref| <= (2 K + 4) u S + 2^-126,   S = sum_k |a_k| |b_k| + |bias|,   u = 2^-24.
"""
from dataclasses import dataclass

import numpy as np
import torch

F32, F64, BF16, I64 = torch.float32, torch.float64, torch.bfloat16, torch.int64
U = 2.0 ** -24        # unit roundoff of fp32
U_BF16 = 2.0 ** -8    # of bf16 (8 significant bits): half an ulp at the foot of a binade, what round to nearest even can miss by
TINY = 2.0 ** -126    # smallest normal fp32: results below it may be flushed
NAN = float("nan")
SENTINEL = -3.0e33    # no result of any case comes near it; bf16 and fp32 both hold a (rounded) copy
LEAKY = float(np.float32(0.01))  # the kernels' and torch's slope is the fp32 constant
ACTS = ["linear", "relu", "leaky_relu", "tanh", "sigmoid", "softplus"]  # index = RG_ACT_*
SMOOTH = ("tanh", "sigmoid", "softplus")


def act64(z, act):
    z = z.double()
    if act == "linear":
        return z
    if act == "relu":
        return z.clamp(min=0)
    if act == "leaky_relu":
        return torch.where(z > 0, z, LEAKY * z)
    if act == "tanh":
        return torch.tanh(z)
    if act == "sigmoid":
        return torch.sigmoid(z)
    return torch.where(z > 20, z, torch.log1p(torch.exp(z.clamp(max=20))))  # softplus, torch's threshold


def dact64(h, act):
    """d act / dz through the activation OUTPUT h, in float64"""
    h = h.double()
    if act == "linear":
        return torch.ones_like(h)
    if act == "relu":
        return (h > 0).double()
    if act == "leaky_relu":
        return torch.where(h > 0, 1.0, LEAKY).double()
    if act == "tanh":
        return 1 - h * h
    if act == "sigmoid":
        return h * (1 - h)
    return -torch.expm1(-h)


def act32(z, act):
    """torch's own fp32 activation"""
    Fn = torch.nn.functional
    return {"linear": lambda t: t, "relu": torch.relu, "leaky_relu": lambda t: Fn.leaky_relu(t, 0.01), "tanh": torch.tanh,
            "sigmoid": torch.sigmoid, "softplus": Fn.softplus}[act](z)


def dact32_from_output(dy, y, act):
    """torch's own fp32 backward through the output, where it has one (softplus: the statement in fp32)"""
    if act == "tanh":
        return torch.ops.aten.tanh_backward(dy, y)
    if act == "sigmoid":
        return torch.ops.aten.sigmoid_backward(dy, y)
    if act == "softplus":
        return dy * -torch.expm1(-y)
    return (dy.double() * dact64(y, act)).float()  # one exact factor, one rounding


def ulp32(t):
    return torch.from_numpy(np.spacing(np.abs(t.double().numpy()).astype(np.float32)).astype(np.float64))


def bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int16) if t.dtype == BF16 else t.view(torch.int32) if t.dtype == F32 else t


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))


def rne(t, dtype):
    """torch's round-to-nearest-even cast of an fp32-exact value"""
    return t.to(F32).to(dtype)


# ---- operands ---------------------------------------------------------------------------------------------------------
def ints(gen, *shape):
    """integers of magnitude 1..4, a zero at about one element in 32"""
    v = torch.randint(1, 5, shape, generator=gen) * (torch.randint(0, 2, shape, generator=gen) * 2 - 1)
    return torch.where(torch.randint(0, 32, shape, generator=gen) == 0, torch.zeros_like(v), v)


ROW_CLASSES = ["ordinary", "large", "small", "zero", "cancel"]   # rows of the A operand
COL_CLASSES = ["ordinary", "large", "small", "zero"]             # rows of the B operand = output columns


def classes(n, names, shift):
    return {c: torch.tensor([r for r in range(n) if (r + shift) % len(names) == k], dtype=torch.long)
            for k, c in enumerate(names)}


def planted(gen, rows, k, names, shift):
    """[rows, k] normal; row classes x 1e4, x 1e-4, all zero, and [v, -v, v, -v, ...] (its products against the paired
    columns of `paired` cancel)"""
    t = torch.randn(rows, k, generator=gen)
    cl = classes(rows, names, shift)
    t[cl["large"]] *= 1e4
    t[cl["small"]] *= 1e-4
    t[cl["zero"]] = 0
    if "cancel" in cl and len(cl["cancel"]):
        v = torch.randn(len(cl["cancel"]), 1, generator=gen) + 2
        sign = torch.tensor([1.0 if j % 2 == 0 else -1.0 for j in range(k)])
        sign[k - 1 if k % 2 else k:] = 0  # an odd last column would not cancel
        t[cl["cancel"]] = v * sign
    return t, cl


def paired(w):
    """equal weights at the columns (2j, 2j + 1): the `cancel` rows meet them"""
    w = w.clone()
    k = w.shape[1] // 2 * 2
    w[:, 1:k:2] = w[:, 0:k:2]
    return w


# ---- views into NaN / sentinel parents ----------------------------------------------------------------------------------
def pitch_for(cols, multiple, on):
    """a row pitch larger than cols: a multiple of `multiple` if on, else not one (and odd when multiple is even)"""
    p = (cols + multiple) // multiple * multiple
    return p if on else p + 1


class Box:
    """[rows, cols] as a view into a filled parent: two rows above and below, a row pitch larger than the width, the
    first element at a 16-byte boundary plus `off` elements"""

    def __init__(self, dev, rows, cols, dtype, pitch, off=0, fill=NAN, src=None):
        assert pitch >= cols
        self.fill, self.geom = fill, ((rows, cols), (pitch, 1), (2 * pitch + 15) // 16 * 16 + off)
        self.buf = torch.full(((rows + 4) * pitch + 32,), fill, dtype=dtype, device=dev)
        self.v = self.buf.as_strided(*self.geom)
        assert (self.v.data_ptr() % 16 == 0) == (off * self.buf.element_size() % 16 == 0)
        if src is not None:
            self.v.copy_(src.to(dtype))
            self.src = self.cpu()

    def cpu(self):
        return self.v.detach().cpu().contiguous()

    def outside_intact(self):
        """every byte of the parent outside the view is what it was filled with (compared as integers)"""
        b = self.buf.detach().cpu().clone()
        b.as_strided(*self.geom).fill_(self.fill)
        return torch.equal(bits(b), bits(torch.full_like(b, self.fill)))

    def unchanged(self):
        return same_bits(self.cpu(), self.src)

    def written(self):
        """an output: no NaN inside and nothing of the sentinel left"""
        c = self.cpu().float()
        return not bool(c.isnan().any()) and not bool((c == torch.tensor(self.fill, dtype=self.buf.dtype).float()).any())


def workspace(dev, nbytes):
    """-> (parent with a sentinel tail of 16 floats, the view of exactly nbytes)"""
    buf = torch.full((nbytes // 4 + 16,), SENTINEL, dtype=F32, device=dev)
    return buf, buf[:nbytes // 4]


@dataclass(frozen=True)
class Layout:
    """the alignment table: where each operand and output of a call lies"""
    a_off: int = 0        # elements the A operand's base lies past a 16-byte boundary
    b_off: int = 0
    a_vec: bool = True    # lda a multiple of VEC
    b_vec: bool = True
    ldy_even: bool = True
    ldyt4: bool = True    # ldyt a multiple of 4 (else odd)
    y32_off: int = 0      # elements y32's base lies past a 16-byte boundary

    @staticmethod
    def of(seed):
        s = int(seed)
        return Layout(s & 1, (s >> 1) & 1, not (s >> 2) & 1, not (s >> 3) & 1, not (s >> 4) & 1, not (s >> 5) & 1, (s >> 6) & 1)


# ---- bounds -----------------------------------------------------------------------------------------------------------
def gemm_statement(a, b, bias=None):
    """float64 product a @ b.T (+ bias) of the operands as stored, and S"""
    a, b = a.double(), b.double()
    ref, S = a @ b.t(), a.abs() @ b.abs().t()
    if bias is not None:
        ref, S = ref + bias.double(), S + bias.double().abs()
    return ref, S


def forward_bound(ref, S, K, act, A_act, bf16_out):
    bd = (2 * K + 4) * U * S + TINY  # relu, leaky_relu, tanh, sigmoid, softplus are Lipschitz 1
    if act == "leaky_relu":
        bd = bd + ulp32(ref)
    if act in SMOOTH:
        bd = bd + A_act[act] * U * ref.abs().clamp(min=TINY)
    return bf16_rounded(bd, ref) if bf16_out else bd


def bf16_rounded(bd, ref):
    """the bound of a bf16 output from that of the fp32 value it is rounded from: |fl(v) - v| <= 2^-8 |v|, |v| <= |ref| + bd"""
    return bd * (1 + U_BF16) + U_BF16 * ref.abs()


def through_output_scale(ref, P, h, act):
    """what the error of act'(h) formed from the stored output is measured against: the result, and for tanh the product's
    h^2 share as well (1 - h * h rounds h * h by u h^2 whatever is subtracted after; torch's tanh_backward does the same)"""
    return ref.abs() + (h.double() ** 2 * P.abs() if act == "tanh" else 0.0)


def dgrad_bound(ref, P, S, h, g, K, act, A_act, bf16_out):
    """P, S: the product before the mask and its sum of magnitudes; h: the stored output of the layer below; g = act'(h)"""
    bd = (2 * K + 4) * U * S * g.abs() + TINY  # (the masked product itself may be flushed, or land on bf16's subnormal grid)
    if act == "leaky_relu":
        bd = bd + ulp32(ref)
    if act in SMOOTH:
        bd = bd + A_act[act] * U * through_output_scale(ref, P, h, act).clamp(min=TINY)
    return bf16_rounded(bd, ref) if bf16_out else bd


def act_backward_bound(ref, dy, y, act, A_act):
    bd = 2 * ulp32(ref)
    if act in SMOOTH:
        bd = bd + A_act[act] * U * through_output_scale(ref, dy.double(), y, act).clamp(min=TINY)
    return bd


def wgrad_bound(S, batch):
    return (2 * batch + 4) * U * S + TINY
