from .graph_workflow import GraphWorkflow  # noqa: F401
