from .make_trainer import make_trainer, make_wrapper  # noqa: F401
