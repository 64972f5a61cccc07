from .distance_transform import DistanceTransformBase, DistanceTransformLocal  # noqa: F401
