from .layer import TernaryConv2dBase
