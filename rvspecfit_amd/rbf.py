"""scipy.interpolate.RBFInterpolator for the subset regularize_grid uses (multiquadric
kernel, degree 0, all nodes), on the device: rvs_rbf_factor / _solve / _eval of
csrc/rbf.hip.  There is no CPU path."""
import numpy as np
import torch

from . import _lib

MAX_N = 16384           # RVS_RBF_MAX_N
# the coefficients of one column chunk: [N, chunk] doubles next to the N^2 factor
CHUNK_BYTES = 1 << 30


class SingularMatrix(np.linalg.LinAlgError):
    """the factorisation met a pivot that is not positive (coincident nodes); scipy
    raises LinAlgError('Singular matrix') there"""


def _dev(a, device, dtype=None):
    if isinstance(a, torch.Tensor):
        t = a.to(device)
    else:
        t = torch.as_tensor(np.ascontiguousarray(a)).to(device)
    if dtype is not None:
        t = t.to(dtype)
    return t.contiguous()


class RBFInterpolator:
    """RBFInterpolator(y, d, smoothing=0.0, kernel='multiquadric', epsilon=1.0) and
    __call__(x), scipy's call form.  y [N, ndim] and x [M, ndim]: numpy arrays or
    tensors; d [N] or [N, S], float32 or float64 (kept as given on the device; the
    arithmetic is float64).  __call__ returns a device tensor [M] or [M, S], float64
    unless out_dtype says torch.float32."""

    def __init__(self, y, d, neighbors=None, smoothing=0.0, kernel='multiquadric',
                 epsilon=1.0, degree=None, device='cuda'):
        if kernel != 'multiquadric':
            raise ValueError("kernel: only 'multiquadric' is built here, got %r"
                             % (kernel, ))
        if neighbors is not None:
            raise ValueError('neighbors is not supported')
        if degree is not None and int(degree) != 0:
            raise ValueError('degree: only 0 (the multiquadric default) is supported')
        epsilon = float(epsilon)
        if not epsilon > 0:
            raise ValueError('epsilon must be positive')
        _lib.require_gpu()
        y = _dev(y, device, torch.float64)
        if y.ndim != 2:
            raise ValueError('`y` must be a 2-dimensional array.')
        N, ndim = y.shape
        d = _dev(d, device)
        if d.dtype != torch.float32:
            d = d.to(torch.float64)
        if d.shape[0] != N:
            raise ValueError('Expected the first axis of `d` to have length %d.' % N)
        self.d_shape = tuple(d.shape[1:])
        d = d.reshape(N, -1)
        if N < 1 or N > MAX_N or not 1 <= ndim <= 8 or d.shape[1] < 1:
            raise ValueError('RBFInterpolator: %d nodes (1 .. %d) of %d dimensions '
                             '(1 .. 8)' % (N, MAX_N, ndim))
        if np.ndim(smoothing) == 0 and not isinstance(smoothing, torch.Tensor):
            smoothing = None if float(smoothing) == 0 else np.full(N, float(smoothing))
        if smoothing is not None:
            smoothing = _dev(smoothing, device, torch.float64)
            if smoothing.shape != (N, ):
                raise ValueError('Expected `smoothing` to be a scalar or have shape '
                                 '(%d,).' % N)
        self.y, self.d, self.epsilon, self.N, self.ndim = y, d, epsilon, N, ndim
        self.S = d.shape[1]
        self.device = y.device
        # column chunk: the coefficients are made chunk by chunk next to the one factor
        self.chunk = int(max(1, min(self.S, CHUNK_BYTES // (8 * max(N, 64)))))
        L = _lib.lib()
        nwork = L.rvs_rbf_work_size(N, self.chunk)
        if nwork < 0:
            raise ValueError('rvs_rbf_work_size: bad shape (N %d, S %d)' % (N, self.chunk))
        self.work = torch.empty(nwork, dtype=torch.float64, device=self.device)
        self.status = torch.zeros(1, dtype=torch.int32, device=self.device)
        rc = L.rvs_rbf_factor(_lib.ptr(y), N, ndim, epsilon, _lib.ptr(smoothing),
                              _lib.ptr(self.work), _lib.ptr(self.status), _lib.stream())
        if rc == -1:
            raise ValueError('rvs_rbf_factor: bad argument')
        _lib.check(rc, 'rvs_rbf_factor')
        self._raise_on_status()
        self._solved = None        # the chunk whose coefficients `work` holds

    def _raise_on_status(self):
        st = int(self.status.item())
        if st & _lib.ST_NONFINITE:
            raise ValueError('RBFInterpolator: the nodes, the smoothing or the values '
                             'are not finite')
        if st & _lib.ST_RBF_NOTPD:
            raise SingularMatrix('Singular matrix: the system of the %d nodes is not '
                                 'positive definite (coincident nodes?)' % self.N)

    def _solve(self, a, b):
        if self._solved == (a, b):
            return
        self._solved = None
        dv = self.d[:, a:b]
        rc = _lib.lib().rvs_rbf_solve(
            ctypes_ptr(dv), int(dv.dtype == torch.float32), self.d.stride(0), self.N,
            b - a, _lib.ptr(self.work), _lib.ptr(self.status), _lib.stream())
        if rc == -1:
            raise ValueError('rvs_rbf_solve: bad argument')
        _lib.check(rc, 'rvs_rbf_solve')
        self._raise_on_status()
        self._solved = (a, b)

    def __call__(self, x, out_dtype=torch.float64, out=None):
        x = _dev(x, self.device, torch.float64)
        if x.ndim != 2 or x.shape[1] != self.ndim:
            raise ValueError('Expected the second axis of `x` to have length %d.'
                             % self.ndim)
        M = x.shape[0]
        if out is None:
            out = torch.empty((M, self.S), dtype=out_dtype, device=self.device)
        elif out.shape != (M, self.S) or out.stride(1) != 1 or \
                out.dtype not in (torch.float32, torch.float64):
            raise ValueError('out: [%d, %d] float32 / float64 with unit column stride'
                             % (M, self.S))
        if M == 0:
            return out.reshape((M, ) + self.d_shape)
        bits = 32 if out.dtype == torch.float32 else 64
        L = _lib.lib()
        for a in range(0, self.S, self.chunk):
            b = min(self.S, a + self.chunk)
            self._solve(a, b)
            rc = L.rvs_rbf_eval(_lib.ptr(x), M, _lib.ptr(self.y), self.N, self.ndim,
                                self.epsilon, _lib.ptr(self.work), b - a, bits,
                                ctypes_ptr(out[:, a:b]), out.stride(0), _lib.stream())
            if rc == -1:
                raise ValueError('rvs_rbf_eval: bad argument (M %d)' % M)
            _lib.check(rc, 'rvs_rbf_eval')
        return out.reshape((M, ) + self.d_shape)


def ctypes_ptr(t):
    """pointer of a tensor view whose rows are strided (a column chunk)"""
    import ctypes
    return ctypes.c_void_p(t.data_ptr())
