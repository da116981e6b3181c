"""Stationary kernels evaluated on grid distances (host NumPy, O(m)).

Paramz-free counterparts of reference runlmc/kern/{rbf,matern32,std_periodic,
scaled,stationary_kern}.py: only ``from_dist``, ``kernel_gradient``,
``update_gradient`` and ``active_dims`` are on the hot path's input side."""
import numpy as np


class StationaryKern:
    """A kernel k(r) of distance with differentiable parameters."""

    def __init__(self, name, active_dims=None):
        self.name = name
        self.active_dims = active_dims
        self.gradient = None

    def from_dist(self, dists):
        raise NotImplementedError

    def kernel_gradient(self, dists):
        """List of dk/dtheta_p arrays, one per parameter."""
        raise NotImplementedError

    def update_gradient(self, grad):
        self.gradient = np.asarray(grad, dtype=float)

    @property
    def param_array(self):
        raise NotImplementedError


class RBF(StationaryKern):
    """exp(-gamma r^2 / 2) (reference rbf.py:39-54)."""

    def __init__(self, inv_lengthscale=1, name='rbf', active_dims=None):
        super().__init__(name, active_dims)
        self.inv_lengthscale = float(inv_lengthscale)

    def from_dist(self, dists):
        return np.exp(-0.5 * np.square(dists) * self.inv_lengthscale)

    def kernel_gradient(self, dists):
        sq = np.square(dists)
        return [np.exp(-0.5 * sq * self.inv_lengthscale) * (-0.5 * sq)]

    @property
    def param_array(self):
        return np.array([self.inv_lengthscale])

    def set_params(self, p):
        self.inv_lengthscale = float(p[0])


class Matern32(StationaryKern):
    """(1 + s) exp(-s), s = sqrt(3) gamma r (reference matern32.py:39-57)."""

    def __init__(self, inv_lengthscale=1, name='matern32', active_dims=None):
        super().__init__(name, active_dims)
        self.inv_lengthscale = float(inv_lengthscale)

    def from_dist(self, dists):
        s = dists * np.sqrt(3) * self.inv_lengthscale
        return (1 + s) * np.exp(-s)

    def kernel_gradient(self, dists):
        root3r = dists * np.sqrt(3)
        s = root3r * self.inv_lengthscale
        e = np.exp(-s)
        return [(1 + s) * (-root3r * e) + root3r * e]

    @property
    def param_array(self):
        return np.array([self.inv_lengthscale])

    def set_params(self, p):
        self.inv_lengthscale = float(p[0])


class Matern52(StationaryKern):
    """(1 + s + s^2 / 3) exp(-s), s = sqrt(5) gamma r: the file's parameter convention
    (Matern32: s = sqrt(3) gamma r); the reference has no such kernel."""

    def __init__(self, inv_lengthscale=1, name='matern52', active_dims=None):
        super().__init__(name, active_dims)
        self.inv_lengthscale = float(inv_lengthscale)

    def from_dist(self, dists):
        s = dists * np.sqrt(5) * self.inv_lengthscale
        return (1 + s + s * s / 3) * np.exp(-s)

    def kernel_gradient(self, dists):
        # dk/dgamma = -(5 gamma r^2 / 3) (1 + s) exp(-s): one product, nothing cancels at r = 0
        root5r = dists * np.sqrt(5)
        s = root5r * self.inv_lengthscale
        return [-(root5r * s / 3) * (1 + s) * np.exp(-s)]

    @property
    def param_array(self):
        return np.array([self.inv_lengthscale])

    def set_params(self, p):
        self.inv_lengthscale = float(p[0])


class StdPeriodic(StationaryKern):
    """exp(-gamma sin^2(pi r / T) / 2) (reference std_periodic.py:44-67)."""

    def __init__(self, inv_lengthscale=1, period=1, name='std_periodic',
                 active_dims=None):
        super().__init__(name, active_dims)
        self.inv_lengthscale = float(inv_lengthscale)
        self.period = float(period)

    def from_dist(self, dists):
        if np.log(self.period) < -200:
            return np.nan
        s = np.sin((np.pi / self.period) * dists)
        return np.exp(-0.5 * np.square(s) * self.inv_lengthscale)

    def kernel_gradient(self, dists):
        arg = np.pi / self.period * dists
        s = np.sin(arg)
        ds = np.cos(arg) * arg * (-1 / self.period * self.inv_lengthscale)
        sq = np.square(s)
        e = np.exp(-0.5 * sq * self.inv_lengthscale)
        return [e * (-0.5 * sq), e * (-1 * s * ds)]

    @property
    def param_array(self):
        return np.array([self.inv_lengthscale, self.period])

    def set_params(self, p):
        self.inv_lengthscale, self.period = float(p[0]), float(p[1])


class Scaled(StationaryKern):
    """scale * k(r); the scale is the LAST parameter (reference
    runlmc/kern/scaled.py:13-37)."""

    def __init__(self, k, scale=1.0):
        super().__init__('scaled_' + k.name, k.active_dims)
        self.k = k
        self.scale = float(scale)

    def from_dist(self, dists):
        return self.scale * self.k.from_dist(dists)

    def kernel_gradient(self, dists):
        return ([self.scale * g for g in self.k.kernel_gradient(dists)] +
                [self.k.from_dist(dists)])

    def update_gradient(self, grad):
        # the reference creates `scale` but never links it (scaled.py:20), so
        # it is not optimised: the free parameters are the inner kernel's
        grad = np.asarray(grad, dtype=float)
        self.gradient = grad[:-1]
        self.scale_gradient = float(grad[-1])
        self.k.update_gradient(grad[:-1])

    @property
    def param_array(self):
        return self.k.param_array

    def set_params(self, p):
        self.k.set_params(p)


class Cosine(StationaryKern):
    """cos(2 pi f r): a rank-2 positive semidefinite kernel (the reference has none); as a
    factor of a Product it makes a spectral-mixture component or a damped cosine."""

    def __init__(self, frequency=1, name='cosine', active_dims=None):
        super().__init__(name, active_dims)
        self.frequency = float(frequency)

    def from_dist(self, dists):
        return np.cos(2 * np.pi * self.frequency * dists)

    def kernel_gradient(self, dists):
        return [-(2 * np.pi * dists) * np.sin(2 * np.pi * self.frequency * dists)]

    @property
    def param_array(self):
        return np.array([self.frequency])

    def set_params(self, p):
        self.frequency = float(p[0])


class Product(StationaryKern):
    """k_1(r) k_2(r) [k_3(r)]: 2 or 3 leaf kernels (RBF, Matern32, Matern52, StdPeriodic,
    Cosine) on ONE Euclidean distance over the product's active dimensions.  Parameters and
    derivatives: the factors in the order given, each factor's in its own order.  A scale goes
    outside: Scaled(Product(...), c)."""

    MAX_FACTORS = 3

    def __init__(self, *factors, name=None, active_dims=None):
        leaves = []
        for f in factors:
            if isinstance(f, Scaled):
                raise ValueError('a Scaled factor in a Product: put the scale outside, '
                                 'Scaled(Product(...), c)')
            if isinstance(f, Product):
                leaves.extend(f.factors)
            elif type(f) in (RBF, Matern32, Matern52, StdPeriodic, Cosine):
                leaves.append(f)
            else:
                raise ValueError('a Product takes RBF, Matern32, Matern52, StdPeriodic and Cosine '
                                 'factors, got %s' % type(f).__name__)
        if len(leaves) < 2:
            raise ValueError('a Product takes at least 2 factors, got %d' % len(leaves))
        if len(leaves) > self.MAX_FACTORS:
            raise ValueError('a Product takes at most %d leaf factors, got %d'
                             % (self.MAX_FACTORS, len(leaves)))
        want = None if active_dims is None else tuple(sorted(active_dims))
        for f in leaves:
            if f.active_dims is not None and tuple(sorted(f.active_dims)) != want:
                raise ValueError('factor %s acts on dimensions %s, the product on %s: every factor '
                                 'takes the product\'s distance' % (f.name, f.active_dims, active_dims))
        self.factors = leaves
        super().__init__(name or '_x_'.join(f.name for f in leaves), active_dims)

    @property
    def active_dims(self):
        return self._active_dims

    @active_dims.setter
    def active_dims(self, value):
        self._active_dims = value
        for f in self.factors:
            f.active_dims = value

    def from_dist(self, dists):
        vals = [f.from_dist(dists) for f in self.factors]
        if any(np.ndim(v) == 0 and np.isnan(v) for v in vals):
            return np.nan       # (StdPeriodic's convention for a vanishing period)
        out = vals[0]
        for v in vals[1:]:
            out = out * v
        return out

    def kernel_gradient(self, dists):
        vals = [f.from_dist(dists) for f in self.factors]
        grads = []
        for i, f in enumerate(self.factors):
            others = 1.0
            for j, v in enumerate(vals):
                if j != i:
                    others = others * v
            grads.extend(g * others for g in f.kernel_gradient(dists))
        return grads

    def _sizes(self):
        return [len(f.param_array) for f in self.factors]

    def update_gradient(self, grad):
        grad = np.asarray(grad, dtype=float)
        self.gradient = grad
        pos = 0
        for f, n in zip(self.factors, self._sizes()):
            f.update_gradient(grad[pos:pos + n])
            pos += n

    @property
    def param_array(self):
        return np.concatenate([f.param_array for f in self.factors])

    def set_params(self, p):
        pos = 0
        for f, n in zip(self.factors, self._sizes()):
            f.set_params(p[pos:pos + n])
            pos += n
