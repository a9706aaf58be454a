"""The reference's make_nd, its --regulargrid branch: the contents of a
specs_<setup>.h5 -> the dictionary a regular-grid TemplateLibrary is made of.  The
Delaunay branch is not here (tools/convert_artefacts.py reads what the reference made).
"""
import numpy as np

from . import read_grid


def regular_library(specs_dict):
    """make_nd.execute(regular=True) (make_nd.py:94-99, 142-170) without its files.
    specs_dict: what make_interpol.build_specs returns.  Returns the converted
    artefact's keys (lam, dats, vec [mapped], idgrid, uvec0.., log_step, log_ids,
    parnames, lognorms, log_spec) that TemplateLibrary, make_ccf.build_ccf_set and the
    test oracle's Library read; `dats` is the rows as given (a device tensor stays
    one)."""
    D = specs_dict
    log_ids = tuple(int(_) for _ in D['mapper_args'][0])
    mapper = read_grid.LogParamMapper(log_ids)
    vec = np.asarray(D['vec']).astype(float)
    vec = mapper.forward(vec)
    if not np.isfinite(vec.sum()):
        raise RuntimeError('Something is broken the parameters are not finite')
    ndim = len(vec[:, 0])
    uvecs0 = [np.unique(vec[i, :], return_inverse=True) for i in range(ndim)]
    uvecs = [_[0] for _ in uvecs0]
    vecids = [np.asarray(_[1]).reshape(-1) for _ in uvecs0]
    lens = [len(_) for _ in uvecs]
    # where each grid point's row is; -1 where the grid has a hole
    idgrid = np.zeros(lens, dtype=int) - 1
    idgrid[tuple(vecids)] = np.arange(vec.shape[1])
    out = dict(lam=np.asarray(D['lam'], dtype=np.float64), dats=D['specs'], vec=vec,
               idgrid=idgrid.astype(np.int64), log_step=np.array(bool(D['log_step'])),
               log_ids=np.array(log_ids, dtype=np.int64),
               parnames=np.array(list(D['parnames'])),
               lognorms=np.asarray(D['lognorms'], dtype=np.float64),
               log_spec=np.array(bool(D.get('log_spec', True))))
    for i, u in enumerate(uvecs):
        out['uvec%d' % i] = u
    return out
