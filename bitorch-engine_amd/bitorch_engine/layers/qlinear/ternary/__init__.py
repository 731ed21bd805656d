from .layer import TernaryLinearBase, TernaryWeightState, ternarize
