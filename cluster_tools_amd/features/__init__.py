from .features_workflow import RegionFeaturesWorkflow  # noqa: F401
