from .postprocess_workflow import SizeFilterWorkflow  # noqa: F401
