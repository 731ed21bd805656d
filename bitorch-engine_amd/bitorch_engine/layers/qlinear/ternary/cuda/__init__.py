from .layer import TernaryLinearCuda
