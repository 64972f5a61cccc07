from .postprocess_workflow import SizeFilterWorkflow  # noqa: F401
from .postprocess_workflow import ConnectedComponentsWorkflow, SizeFilterAndGraphWatershedWorkflow  # noqa: F401
from .graph_connected_components import GraphConnectedComponentsLocal  # noqa: F401
from .graph_watershed_assignments import GraphWatershedAssignmentsLocal  # noqa: F401
