from .distance_transform import DistanceTransformBase, DistanceTransformLocal  # noqa: F401
from .seeds import WatershedSeedsBase, WatershedSeedsLocal  # noqa: F401
