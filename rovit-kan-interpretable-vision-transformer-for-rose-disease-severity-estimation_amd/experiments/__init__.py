from .compare import compare_models

__all__ = ['compare_models']
