from .find_uniques import FindUniquesLocal  # noqa: F401
