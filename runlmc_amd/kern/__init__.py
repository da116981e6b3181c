"""Stationary kernels of the latent processes."""
from .stationary import (StationaryKern, RBF, Matern32, Matern52, StdPeriodic, Cosine, Product,
                         Scaled, Separable, Lags)

__all__ = ['StationaryKern', 'RBF', 'Matern32', 'Matern52', 'StdPeriodic', 'Cosine', 'Product',
           'Scaled', 'Separable', 'Lags']
