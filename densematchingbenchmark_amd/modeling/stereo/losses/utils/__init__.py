from .quantile_loss import quantile_loss

__all__ = ["quantile_loss"]
