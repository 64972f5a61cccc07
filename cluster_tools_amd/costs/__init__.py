from .costs_workflow import EdgeCostsWorkflow  # noqa: F401
