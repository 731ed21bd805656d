from .layer import TernaryLinearBase, ternarize
