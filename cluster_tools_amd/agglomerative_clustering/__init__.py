from .agglomerative_clustering import AgglomerativeClusteringLocal  # noqa: F401
