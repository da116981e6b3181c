from .likelihood import ExactLMCLikelihood  # noqa: F401
