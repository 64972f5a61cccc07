from .node_label_workflow import NodeLabelWorkflow  # noqa: F401
