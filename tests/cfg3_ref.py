"""Three-branch classifier-free guidance restated for the tests: the float64 formula, the torch fp32 expression the kernel must reproduce bit
for bit, the rounding bound between the three-branch form at s_l == s_t and the two-branch form, and the rule that says which steps need the
text-only branch.  Nothing here imports the package."""
import numpy as np

EPS32 = 2.0 ** -24          # unit roundoff of float32


def combine2(e_c, e_u, g):
    """today's guidance: e = e_u + g (e_c - e_u)"""
    return e_u + g * (e_c - e_u)


def combine3(e_c, e_t, e_u, s_text, s_layout):
    """e = (e_u + s_t (e_t - e_u)) + s_l (e_c - e_t), left to right (float64 arrays in, float64 out)"""
    return (e_u + s_text * (e_t - e_u)) + s_layout * (e_c - e_t)


def torch_combine3(eps3b, s_text, s_layout):
    """the torch fp32 expression over the thirds of eps3b [3n, ...] = [cond ; text-only ; uncond]: one rounding per operation, no contraction"""
    e_c, e_t, e_u = eps3b.chunk(3, 0)
    return (e_u + s_text * (e_t - e_u)) + s_layout * (e_c - e_t)


def same_scale_bound(e_c, e_t, e_u, s):
    """|combine3(s, s) - combine2(s)| in fp32, elementwise.  In exact arithmetic the two agree (e_t cancels).  In fp32 each form rounds
    every operation once: the three-branch form has 6 operations whose operands are bounded by |e_u| + s (|e_t| + |e_u|) and s (|e_c| + |e_t|),
    the two-branch form 3 bounded by |e_u| + s (|e_c| + |e_u|); first-order error <= 2^-24 times the sum of the magnitudes each rounding sees,
    which the factor 8 over |e_u| + s (|e_c| + 2 |e_t| + |e_u|) covers with room for the second-order terms."""
    return 8.0 * EPS32 * (np.abs(e_u) + s * (np.abs(e_c) + 2.0 * np.abs(e_t) + np.abs(e_u)))


def needs_text_branch(relation: bool, fuser_scale: float) -> bool:
    """a step sees the grounding through the gated self-attention (skipped at fuser scale 0) and, on a relation model, through the relation
    chain at every scale"""
    return bool(relation) or fuser_scale != 0
