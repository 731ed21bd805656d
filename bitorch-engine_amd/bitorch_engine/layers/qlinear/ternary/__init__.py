from .layer import TernaryLinearBase, TernaryWeightState, ternarize, ternarize_absmean
