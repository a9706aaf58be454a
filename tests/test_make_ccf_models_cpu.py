"""Host side of building CCF template sets (make_ccf.build_ccf_set): the Morton-curve
selection against the sets the reference made, the spline / bin tables of the
template grids (26 and 40 nodes) against scipy, and the new export."""
import os
import re

import numpy as np
import pytest

from rvspecfit_amd import ccf_tables, make_ccf

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(REPO, 'tests', 'golden')
LIBS = ('lib_gold_b', 'lib_gold_r', 'lib_desi_b', 'lib_desi_r', 'lib_desi_z')


@pytest.mark.parametrize('name', LIBS)
def test_selection_reproduces_the_reference_sets(name):
    """rvs_make_ccf --every 20 --vsinis 0,100 chose these templates: the same rows, in
    the same order, from the library's mapped `vec` (dense ranks do not see log10)"""
    d = np.load(os.path.join(GOLD, name + '.npz'))
    vec = d['vec']
    inds = make_ccf.select_templates(vec, 20)
    assert len(inds) * 2 == len(d['ccf_params'])
    par = vec.T[inds].copy()
    for i in np.atleast_1d(d['log_ids']):
        par[:, i] = 10**par[:, i]
    want = d['ccf_params'][::2]
    assert np.array_equal(d['ccf_params'][::2], d['ccf_params'][1::2])
    logc = np.zeros(par.shape[1], dtype=bool)
    logc[np.atleast_1d(d['log_ids'])] = True
    assert np.array_equal(par[:, ~logc], want[:, ~logc])        # exact
    # (10**log10(Teff) is Teff to an ulp or two)
    assert np.allclose(par[:, logc], want[:, logc], rtol=1e-13, atol=0)
    assert np.array_equal(d['ccf_vsinis'], np.tile([0., 100.], len(inds)))
    # the physical parameters give the same order
    phys = vec.copy()
    for i in np.atleast_1d(d['log_ids']):
        phys[i] = 10**phys[i]
    assert np.array_equal(make_ccf.select_templates(phys, 20), inds)


def test_morton_numbers_of_small_grids_worked_by_hand():
    """2 x 2: a coordinate is 0 or 1, 1 falls into the last of the 2^32 cells (all bits
    set), x takes the even places and y the odd ones.  4 x 4: the ranks 0, 1/3, 2/3, 1
    are the cells 0x00000000, 0x55555555, 0xAAAAAAAA, 0xFFFFFFFF, whose two leading
    bits are the rank itself, so the numbers, read unsigned, walk the textbook Z; read
    as int64 (what np.argsort sees, as in the reference) the upper half, y >= 2, has
    the sign bit and comes first."""
    ids = make_ccf.get_mortoncurve_id(np.array([[0., 0.], [1., 0.], [0., 1.], [1., 1.]]))
    assert ids.dtype == np.int64
    assert [int(_) for _ in ids.view(np.uint64)] == [0, 0x5555555555555555,
                                                     0xAAAAAAAAAAAAAAAA,
                                                     0xFFFFFFFFFFFFFFFF]
    # values that are not ranks give the same numbers: only their order enters
    ids2 = make_ccf.get_mortoncurve_id(np.array([[3.5, -2.], [9., -2.], [3.5, 40.],
                                                 [9., 40.]]))
    assert np.array_equal(ids, ids2)
    pts = np.array([[x, y] for y in range(4) for x in range(4)], dtype=float)
    ids = make_ccf.get_mortoncurve_id(pts)
    z = [(0, 0), (1, 0), (0, 1), (1, 1), (2, 0), (3, 0), (2, 1), (3, 1),
         (0, 2), (1, 2), (0, 3), (1, 3), (2, 2), (3, 2), (2, 3), (3, 3)]
    walk = pts[np.argsort(ids.view(np.uint64))]
    assert [tuple(int(c) for c in p) for p in walk] == z
    signed = pts[np.argsort(ids)]
    assert [tuple(int(c) for c in p) for p in signed] == z[8:] + z[:8]
    # three dimensions: 21 bits each, the corner (1, 1, 1) sets the low 63 bits
    c3 = make_ccf.get_mortoncurve_id(np.array([[0., 0., 0.], [1., 1., 1.], [1., 0., 0.],
                                               [0., 0., 1.]]))
    assert int(c3[1]) == 2**63 - 1
    assert int(c3[2]) == sum(1 << (3 * j) for j in range(21))
    assert int(c3[3]) == sum(1 << (3 * j + 2) for j in range(21))


def test_selection_equal_keys_and_large_every():
    # repeated parameter vectors: equal Morton numbers, np.argsort's order
    X = np.array([[0., 0.], [1., 1.], [0., 0.], [1., 0.], [1., 1.], [0., 1.]])
    ids = make_ccf.get_mortoncurve_id(X)
    assert ids[0] == ids[2] and ids[1] == ids[4]
    assert np.array_equal(make_ccf.select_templates(X.T, 1), np.argsort(ids))
    # every beyond the grid: the first template of the curve alone
    assert np.array_equal(make_ccf.select_templates(X.T, 1000), np.argsort(ids)[:1])


def test_single_valued_dimension_is_an_error():
    X = np.array([[0., 5.], [1., 5.], [2., 5.]])
    with pytest.raises(ValueError, match='single value'):
        make_ccf.get_mortoncurve_id(X)


def _scipy_continuum(nodes, p, lam):
    import scipy.interpolate
    return scipy.interpolate.UnivariateSpline(nodes, p, s=0, k=2)(lam)


@pytest.mark.parametrize('name,nfold', [('lib_gold_b', 1), ('lib_desi_r', 1),
                                        ('lib_gold_b', 0)])
def test_template_grid_tables_against_scipy(name, nfold):
    """the template grid is wider than the CCF range by the velocity padding: 26
    nodes on the committed libraries (more than a spectrum's 24), 40 on a grid
    stretched to that many node steps"""
    d = np.load(os.path.join(GOLD, name + '.npz'))
    lam = d['lam']
    step = float(d['ccf_splinestep'])
    if nfold == 0:       # a grid of 40 nodes
        lam = lam[0] * np.exp(np.linspace(0, 39.5 * np.log(1 + step / 3e5), 5000))
    cc = dict(logl0=float(d['ccf_logl0']), logl1=float(d['ccf_logl1']), npoints=1024,
              continuum=True, splinestep=step)
    T = make_ccf.model_tables(lam, cc)
    m = T['nnode']
    assert (24 < m <= 26) if nfold else m == 40
    nodes = T['nodes']
    N = int(np.ceil(np.log(lam.max() / lam.min()) / np.log(1 + step / 3e5)))
    assert m == N and nodes[0] == lam.min()
    rng = np.random.default_rng(m)
    p = rng.normal(size=m)
    c = T['Cinv'][0] @ p
    S = np.array([T['Eb'][k] @ c[T['El'][k]:T['El'][k] + 3] for k in range(len(lam))])
    want = _scipy_continuum(nodes, p, lam)
    assert np.max(np.abs(S - want)) < 1e-11 * np.max(np.abs(want))
    assert np.allclose(T['Cinv'][1] @ T['Cinv'][0], np.eye(m), atol=1e-10)
    # knot intervals and bins partition the pixels
    ist, bst = T['istart'], T['bin_start']
    assert ist[0] == 0 and ist[m - 2] == len(lam) and np.all(np.diff(ist) >= 0)
    assert np.all(T['El'] >= 0) and np.all(T['El'] <= m - 3)
    import scipy.stats
    _, edges = ccf_tables.continuum_nodes(lam, step)
    bs = scipy.stats.binned_statistic(lam, lam, 'count', bins=edges)
    assert np.array_equal(np.diff(bst), bs.statistic.astype(int))
    assert bst[0] >= 0 and bst[-1] <= len(lam)
    # interp1d's bracket: -1 outside the row, else lam[hi - 1] < x <= lam[hi]
    ihi, logl, lnl = T['ihi'], T['logl'], T['lnlam']
    ins = ihi >= 0
    assert np.all(ihi[ins] >= 1) and np.all(ihi[ins] <= len(lam) - 1)
    assert np.all(lnl[ihi[ins] - 1] <= logl[ins]) and np.all(logl[ins] <= lnl[ihi[ins]])
    assert np.all((logl[~ins] < lnl[0]) | (logl[~ins] > lnl[-1]))


def test_row_and_node_limits_are_errors_before_any_launch():
    cc = dict(logl0=8.3, logl1=8.4, npoints=1024, continuum=True, splinestep=1000.)
    lam = 4000 * np.exp(np.arange(make_ccf.MODEL_MAX_NTP + 1) * 1e-5)
    with pytest.raises(ValueError, match='at most'):
        make_ccf.model_tables(lam, cc)
    make_ccf.model_tables(lam[:-1], cc)
    with pytest.raises(ValueError, match='nodes'):
        make_ccf.model_tables(lam[:6000], dict(cc, splinestep=300.))   # 60 nodes


def test_export_header_and_integration_prototype():
    from rvspecfit_amd import _lib
    L = _lib.lib()
    assert hasattr(L, 'rvs_ccf_models_build') and hasattr(L, 'rvs_ccf_model_rows')
    hdr = open(os.path.join(REPO, 'include', 'rvsgpu.h')).read()
    doc = open(os.path.join(REPO, 'INTEGRATION.md')).read()
    assert int(re.search(r'#define RVS_ABI_VERSION (\d+)', hdr).group(1)) >= 15
    lim = int(re.search(r'#define RVS_CCF_MODEL_MAX_NTP (\d+)', hdr).group(1))
    assert lim == make_ccf.MODEL_MAX_NTP >= 8192
    norm = lambda t: re.sub(r'\s+', ' ', t).strip()
    proto = re.search(r'int rvs_ccf_models_build\([^;]*\);', hdr).group(0)
    assert norm(proto) in norm(doc)
    # argument errors come back as RVS_E_ARG, nothing is launched
    x = np.zeros(8)
    P = x.ctypes.data
    args = lambda ntp, nnode, npts, fft: (
        P, None, None, ntp, 1, 1, P, P, P, P, nnode, P, P, P, P, npts, P, P, fft, fft,
        None, None, None, None)
    assert L.rvs_ccf_models_build(*args(lim + 1, 26, 1024, None)) == -1
    assert L.rvs_ccf_models_build(*args(11, 26, 1024, None)) == -1
    assert L.rvs_ccf_models_build(*args(1000, 49, 1024, None)) == -1
    assert L.rvs_ccf_models_build(*args(1000, 26, 1000, P)) == -1   # not a power of two
    assert L.rvs_ccf_model_rows(None, 1, P, 1, 10, 1, P, None) == -1
