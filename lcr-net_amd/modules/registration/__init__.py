from .matching import get_node_correspondences  # noqa: F401
from .matching import get_node_correspondences_batched  # noqa: F401
from .superpoint_target import SuperPointTargetGenerator  # noqa: F401
