from .distance_transform import DistanceTransformBase, DistanceTransformLocal  # noqa: F401
from .seeds import WatershedSeedsBase, WatershedSeedsLocal  # noqa: F401
from .watershed import WatershedBase, WatershedLocal  # noqa: F401
