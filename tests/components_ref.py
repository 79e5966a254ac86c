"""A float32 numpy restatement of component frames (include/frayhip.h "component frames"): what k_acc_resolve_terms_split makes of a sample's
term list.  Every operation is one float32 operation in the header's order; the states and their outputs are samples_ref's accumulate and
mean_and_noise over the d_i and the n_i."""
import numpy as np

from samples_ref import accumulate, mean_and_noise          # noqa: F401 -- the states of the components are the resumable frames' states

F32 = np.float32


def _terms(terms):
    terms = np.asarray(terms)
    assert terms.dtype == F32 and terms.ndim >= 2 and terms.shape[0] >= 1 and terms.shape[-1] == 3, (terms.dtype, terms.shape)
    return terms


def fold(terms):
    """terms float32 [n, ..., 3], n >= 1: the colour the frame's resolve adds for the sample -- from c3(0, 0, 0), result = t[k] + result for
    k = n-1 .. 0."""
    terms = _terms(terms)
    result = np.zeros(terms.shape[1:], F32)
    for k in range(terms.shape[0] - 1, -1, -1):
        result = terms[k] + result
    return result


def split(terms):
    """(d, n) of a sample: d = t[0] as it is stored, n = the fold of t[1 .. n-1] from c3(0, 0, 0) -- (0, 0, 0) when there is one term."""
    terms = _terms(terms)
    n = np.zeros(terms.shape[1:], F32)
    for k in range(terms.shape[0] - 1, 0, -1):
        n = terms[k] + n
    return terms[0].copy(), n
