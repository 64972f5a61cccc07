from .multicut_workflow import MulticutWorkflow  # noqa: F401
