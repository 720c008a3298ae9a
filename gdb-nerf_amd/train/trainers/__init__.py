from .make_trainer import make_wrapper  # noqa: F401
