from .morphology_workflow import MorphologyWorkflow  # noqa: F401
