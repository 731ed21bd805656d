from .layer import TernaryLinearCuda
from .a8_layer import TernaryA8LinearCuda
