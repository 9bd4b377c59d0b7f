"""CliffordAlgebra nn.Module with the reference's surface
(csmpn/algebra/cliffordalgebra.py:10-262): same buffers (metric, subspaces,
bbo_grades, even_grades, odd_grades, cayley), attributes and method names, so the
reference's models and checkpoints work unchanged.

What differs is where the work happens:
  * the tables come from the native library (csmpn_algebra_tables);
  * geometric_product on GPU tensors runs the sign-table HIP kernel
    (csmpn_geometric_product_*), D^2 products per row instead of a dense D^3 einsum;
  * q / norm use the closed form q_g = sum_d qsign_d x_d^2 (the reference's
    cayley[:, 0, :] slice is diagonal), elementwise on whatever device x is on.
The fused CEMLP / EGCL kernels never call these Python methods.
"""
import functools
import math

import torch
from torch import nn

from csmpn_hip import native, ops

from .metric import ShortLexBasisBladeOrder, gmt_element, native_tables


class CliffordAlgebra(nn.Module):
    def __init__(self, metric):
        super().__init__()
        self.register_buffer("metric", torch.as_tensor(metric))
        self.num_bases = len(metric)
        self.dim = self.num_bases
        self.metric_tuple = tuple(float(m) for m in metric)
        tables = native_tables(self.metric_tuple)
        self.bbo = ShortLexBasisBladeOrder(self.num_bases)
        self.n_blades = 1 << self.dim
        self.grades = self.bbo.grades.unique()
        self.n_subspaces = len(self.grades)
        dflt = torch.get_default_dtype()
        self.register_buffer("subspaces", torch.from_numpy(tables["subspaces"]).clone())
        starts = [0]
        for g in range(self.dim + 1):
            starts.append(starts[-1] + math.comb(self.dim, g))
        self.grade_to_slice = [slice(starts[g], starts[g + 1]) for g in range(self.dim + 1)]
        self.grade_to_index = [torch.arange(starts[g], starts[g + 1]) for g in range(self.dim + 1)]
        self.register_buffer("bbo_grades", self.bbo.grades.to(dflt))
        self.register_buffer("even_grades", self.bbo_grades % 2 == 0)
        self.register_buffer("odd_grades", ~self.even_grades)
        self.register_buffer("cayley", torch.from_numpy(tables["cayley"]).to(dflt))
        self._paths = torch.from_numpy(tables["paths"]).bool()
        g = self.bbo.grades
        beta = torch.where(((g * (g - 1)) // 2) % 2 == 0, 1.0, -1.0)
        diag = torch.from_numpy(tables["cayley"])[torch.arange(self.n_blades), 0, torch.arange(self.n_blades)]
        self._qsign_host = (beta * diag).to(dflt)   # beta_d * cayley[d, 0, d]
        self.hip_supported = bool(native.lib().csmpn_metric_supported(native.metric_array(self.metric_tuple), self.dim))
        # every signature of +1 / -1 entries on 2..5 generators: CEMLP and EGCL run on the device (the run-time-signature
        # kernels where the algebra is not one of the six compiled ones); hip_supported stays the six, which the geometric
        # product and the small layers need
        self.hip_signature = bool(native.lib().csmpn_signature_supported(native.metric_array(self.metric_tuple), self.dim))

    # ------------------------------------------------------------------ products
    def geometric_product(self, a, b, blades=None):
        if blades is None and a.is_cuda and self.hip_supported and a.dtype == torch.float32:
            return ops.geometric_product_apply(a, b, self.metric_tuple)
        cayley = self.cayley
        if blades is not None:
            bl, bo, br = blades
            assert isinstance(bl, torch.Tensor) and isinstance(bo, torch.Tensor) and isinstance(br, torch.Tensor)
            cayley = cayley[bl[:, None, None], bo[:, None], br]
        return torch.einsum("...i,ijk,...k->...j", a, cayley, b)

    def sandwich(self, u, v, w):
        return self.geometric_product(self.geometric_product(u, v), w)

    def reduce_geometric_product(self, inputs):
        return functools.reduce(self.geometric_product, inputs)

    # ------------------------------------------------------------------ involutions
    def _grade_signs(self, exponent, mv):
        return torch.pow(-1, exponent).to(device=mv.device, dtype=mv.dtype)

    def alpha(self, mv, blades=None):
        s = self._grade_signs(self.bbo_grades, mv)
        return (s if blades is None else s[blades]) * mv.clone()

    def beta(self, mv, blades=None):
        s = self._grade_signs(self.bbo_grades * (self.bbo_grades - 1) / 2, mv)
        return (s if blades is None else s[blades]) * mv.clone()

    def gamma(self, mv, blades=None):
        s = self._grade_signs(self.bbo_grades * (self.bbo_grades + 1) / 2, mv)
        return (s if blades is None else s[blades]) * mv.clone()

    def zeta(self, mv):
        return mv[..., :1]

    # ------------------------------------------------------------------ embedding / projection
    # (cliffordalgebra.py:98-117; blades are grade-sorted, so a grade is one contiguous slice)
    def _scatter_blades(self, values, where, dtype):
        out = values.new_zeros(values.shape[:-1] + (self.n_blades,), dtype=dtype)
        out[..., where] = values.to(dtype)
        return out

    def embed(self, tensor, tensor_index):
        return self._scatter_blades(tensor, tensor_index, tensor.dtype)

    def embed_grade(self, tensor, grade):
        # the reference allocates in the default dtype whatever the input's: kept
        return self._scatter_blades(tensor, self.grade_to_slice[grade], torch.get_default_dtype())

    def get(self, mv, blade_index):
        return mv[..., tuple(blade_index)]

    def get_grade(self, mv, grade):
        return mv[..., self.grade_to_slice[grade]]

    # ------------------------------------------------------------------ bilinear form, norms
    def b(self, x, y, blades=None):
        if blades is not None:
            assert len(blades) == 2
            bl, br = blades
            sub = self.cayley[bl[:, None], 0, br[None, :]].to(x.dtype)
            return torch.einsum("...i,ik,...k->...", self.beta(x, blades=bl), sub, y)[..., None]
        sub = self.cayley[:, 0, :].to(x.dtype)
        return torch.einsum("...i,ik,...k->...", self.beta(x), sub, y)[..., None]

    def _qsign(self, like):
        return self._qsign_host.to(device=like.device, dtype=like.dtype)

    def q(self, mv, blades=None):
        s = self._qsign(mv)
        if blades is not None:
            s = s[blades]
        return (s * mv * mv).sum(dim=-1, keepdim=True)

    def _smooth_abs_sqrt(self, input, eps=1e-16):
        return (input**2 + eps) ** 0.25

    def norm(self, mv, blades=None):
        return self._smooth_abs_sqrt(self.q(mv, blades=blades))

    def qs(self, mv, grades=None):
        grades = self.grades if grades is None else grades
        return [self.q(self.get_grade(mv, int(g)), blades=self.grade_to_index[int(g)]) for g in grades]

    def norms(self, mv, grades=None):
        grades = self.grades if grades is None else grades
        return [self.norm(self.get_grade(mv, int(g)), blades=self.grade_to_index[int(g)]) for g in grades]

    # (The reference's sampling / versor helpers - random_vector, parity, eta, alpha_w, inverse, rho, versor, rotor,
    # cliffordalgebra.py:170-236 - are not part of the message-passing path and no task model calls them; they are not
    # restated here. SURVEY.md Appendix C lists `inverse` / `rho` as wrong for non-blade versors anyway.)

    # ------------------------------------------------------------------ structure
    @functools.cached_property
    def geometric_product_paths(self):
        return self._paths.clone()

    def split(self, mv):
        return mv.reshape(mv.shape[0], -1, self.n_blades)

    def flatten(self, mv):
        return mv.reshape(mv.shape[0], -1)
