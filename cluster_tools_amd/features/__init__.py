from .features_workflow import EdgeFeaturesWorkflow, RegionFeaturesWorkflow  # noqa: F401
