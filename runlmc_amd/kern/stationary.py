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

    # -- evaluation at per-axis lags: `lags` holds one array of absolute coordinate differences
    #    per active dimension, in sorted order, broadcasting against each other.  A kernel of one
    #    distance forms the Euclidean norm; Separable hands each factor its own axes
    def from_lags(self, lags):
        return self.from_dist(lags_to_dist(lags))

    def kernel_gradient_lags(self, lags):
        return self.kernel_gradient(lags_to_dist(lags))

    @property
    def separable(self):
        """Whether the kernel needs per-axis lags (no single distance determines it)."""
        return False

    def update_gradient(self, grad):
        self.gradient = np.asarray(grad, dtype=float)

    @property
    def param_array(self):
        raise NotImplementedError


def lags_to_dist(lags):
    """r = sqrt(sum lags^2), summed in the order given."""
    return np.sqrt(sum(np.square(np.asarray(g, dtype=float)) for g in lags))


class Lags:
    """Distances that keep their axes: `lags`, one array of absolute coordinate differences per
    active dimension (sorted order, broadcasting against each other), and `dist`, their
    Euclidean norm (an array handed in is kept as it is: a model's kernels of one distance then
    see the array they have always seen).  Accepted wherever the model layers take an array of
    distances (kernel_values / kernel_gradients below)."""

    def __init__(self, lags, dist=None):
        self.lags = tuple(np.asarray(g, dtype=float) for g in lags)
        if not self.lags:
            raise ValueError('Lags needs at least one axis')
        self.dist = lags_to_dist(self.lags) if dist is None else dist

    @property
    def shape(self):
        return np.shape(self.dist)

    @property
    def ndim(self):
        return np.ndim(self.dist)

    @classmethod
    def zero(cls, naxes):
        """Lag zero on every axis (k(0): the native variance)."""
        return cls((np.zeros(()),) * int(naxes), 0)

    @classmethod
    def between(cls, A, B, dist=None):
        """Pairwise lags |a_i - b_j| per column of A (na, p) and B (nb, p)."""
        A, B = np.asarray(A, dtype=float), np.asarray(B, dtype=float)
        return cls([np.abs(A[:, None, c] - B[None, :, c]) for c in range(A.shape[1])], dist)


def kernel_values(k, d):
    """k at `d`: an array of distances (from_dist -- a Separable raises ValueError there) or a
    Lags (a separable kernel takes its axes, any other its distance array)."""
    if isinstance(d, Lags):
        return k.from_lags(d.lags) if getattr(k, 'separable', False) else k.from_dist(d.dist)
    return k.from_dist(d)


def kernel_gradients(k, d):
    """kernel_values' rule for the parameter derivatives."""
    if isinstance(d, Lags):
        return (k.kernel_gradient_lags(d.lags) if getattr(k, 'separable', False)
                else k.kernel_gradient(d.dist))
    return k.kernel_gradient(d)


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

    @staticmethod
    def ard(inv_lengthscales, active_dims):
        """exp(-sum_i gamma_i d_i^2 / 2), an inverse lengthscale per dimension (automatic
        relevance determination): the Separable of one RBF per dimension, 2 or 3 of them."""
        gammas, dims = list(inv_lengthscales), list(active_dims)
        if len(gammas) != len(dims):
            raise ValueError('RBF.ard: %d inverse lengthscales for %d dimensions' % (len(gammas), len(dims)))
        if len(dims) not in (2, 3):
            raise ValueError('RBF.ard takes 2 or 3 dimensions, got %d' % len(dims))
        return Separable(*[RBF(g, name='rbf%d' % d, active_dims=[d]) for g, d in zip(gammas, dims)],
                         name='rbf_ard')


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

    def from_lags(self, lags):
        return self.scale * self.k.from_lags(lags)

    def kernel_gradient_lags(self, lags):
        return ([self.scale * g for g in self.k.kernel_gradient_lags(lags)] +
                [self.k.from_lags(lags)])

    @property
    def separable(self):
        return self.k.separable

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


class Separable(StationaryKern):
    """prod_g k_g(|x - x'| over g's own dimensions): every factor a leaf (RBF, Matern32, Matern52,
    StdPeriodic, Cosine) or a Product of leaves, with an explicit active_dims of its own; the sets
    are pairwise disjoint and their sorted union is the kernel's active_dims.  At least 2 factors,
    at most 3 leaves in all.  Parameters and derivatives as Product's: the factors in the order
    given, each factor's in its own order.  A scale goes outside: Scaled(Separable(...), c).
    There is no single distance: from_lags / kernel_gradient_lags evaluate it, from_dist and
    kernel_gradient raise ValueError."""

    MAX_LEAVES = 3

    def __init__(self, *factors, name=None):
        leaves, seen = 0, {}
        for f in factors:
            if isinstance(f, Scaled):
                raise ValueError('a Scaled factor (%s) in a Separable: put the scale outside, '
                                 'Scaled(Separable(...), c)' % f.name)
            if type(f) is Product:
                leaves += len(f.factors)
            elif type(f) in (RBF, Matern32, Matern52, StdPeriodic, Cosine):
                leaves += 1
            else:
                raise ValueError('a Separable takes RBF, Matern32, Matern52, StdPeriodic, Cosine and '
                                 'Product factors, got %s' % type(f).__name__)
            if f.active_dims is None or len(f.active_dims) == 0:
                raise ValueError('factor %s of a Separable has no active_dims: every factor names '
                                 'its own dimensions' % f.name)
            for d in f.active_dims:
                if int(d) in seen:
                    raise ValueError('factors %s and %s of a Separable both act on dimension %d: the '
                                     'sets must be disjoint' % (seen[int(d)], f.name, int(d)))
            for d in f.active_dims:
                seen[int(d)] = f.name
        if len(factors) < 2:
            raise ValueError('a Separable takes at least 2 factors, got %d' % len(factors))
        if leaves > self.MAX_LEAVES:
            raise ValueError('a Separable takes at most %d leaf kernels in all, got %d'
                             % (self.MAX_LEAVES, leaves))
        self.factors = list(factors)
        for f in self.factors:
            f.active_dims = tuple(sorted(int(d) for d in f.active_dims))
        self._dims = tuple(sorted(seen))
        super().__init__(name or '_x_'.join(f.name for f in self.factors), self._dims)

    @property
    def active_dims(self):
        return self._dims

    @active_dims.setter
    def active_dims(self, value):
        # (FunctionalKernel.set_input_dim writes the sorted tuple back; the factors fix the set)
        if value is not None and tuple(sorted(value)) != self._dims:
            raise ValueError('%s acts on dimensions %s, the union of its factors\': they cannot be '
                             'set to %s' % (self.name, self._dims, tuple(value)))

    @property
    def separable(self):
        return True

    def _no_distance(self):
        raise ValueError('%s is separable: it has no single distance, evaluate it at per-axis lags '
                         '(from_lags, kernel_gradient_lags)' % self.name)

    def from_dist(self, dists):
        self._no_distance()

    def kernel_gradient(self, dists):
        self._no_distance()

    def _own(self, f, lags):
        if len(lags) != len(self._dims):
            raise ValueError('%s acts on %d dimensions, got %d lag arrays'
                             % (self.name, len(self._dims), len(lags)))
        return tuple(lags[self._dims.index(d)] for d in f.active_dims)

    def from_lags(self, lags):
        vals = [f.from_lags(self._own(f, lags)) for f in self.factors]
        if any(np.ndim(v) == 0 and np.isnan(v) for v in vals):
            return np.nan       # (StdPeriodic's convention for a vanishing period)
        out = vals[0]
        for v in vals[1:]:
            out = out * v
        return out

    def kernel_gradient_lags(self, lags):
        vals = [f.from_lags(self._own(f, lags)) for f in self.factors]
        grads = []
        for i, f in enumerate(self.factors):
            others = 1.0
            for j, v in enumerate(vals):
                if j != i:
                    others = others * v
            grads.extend(g * others for g in f.kernel_gradient_lags(self._own(f, lags)))
        return grads

    def leaves(self):
        """(leaf kernel, its dimensions) in derivative order."""
        out = []
        for f in self.factors:
            for leaf in (f.factors if type(f) is Product else [f]):
                out.append((leaf, f.active_dims))
        return out

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
