from .layer import TernaryConv2dCuda
