"""A null-safe reader over a parsed YAML tree: the settings files of the reference (network/config/*.yaml) read the way its
`network.config.Reader` reads them.

    cfg = config.load("MaskFlownet_S.yaml")
    cfg.optimizer.learning_rate.value        # the schedule; raises KeyError when the file has none
    cfg.optimizer.q.get(None)                # None: the file has no `q`
    getattr(cfg.network, "class").get()      # 'class' is a keyword, so getattr

Attribute chaining never raises: a key that is missing, a null node and anything below either are all "absent" nodes.  `.get(default)`
returns the default for an absent node, `.value` raises for one (the reference's hands back None there and fails later, wherever the
None is first used).  The package ships no settings file: `load` takes a path."""


class Reader:
    __slots__ = ("_node", "_path")

    def __init__(self, node, path=""):
        object.__setattr__(self, "_node", node)
        object.__setattr__(self, "_path", path)

    def __getattr__(self, name):
        if name.startswith("__") and name.endswith("__"):      # copy / pickle probes: not keys of a settings file
            raise AttributeError(name)
        node = self._node
        child = node.get(name) if isinstance(node, dict) else None
        return Reader(child, (self._path + "." + name) if self._path else name)

    def __setattr__(self, name, value):
        raise AttributeError("config.Reader is read-only")

    def get(self, default=None):
        return default if self._node is None else self._node

    @property
    def present(self):
        return self._node is not None

    @property
    def value(self):
        if self._node is None:
            raise KeyError("the configuration has no value at '%s'" % self._path)
        return self._node

    def __repr__(self):
        return "Reader(%s=%r)" % (self._path or "<root>", self._node)


def load(path):
    """The YAML file at `path` as a Reader (an empty file is an empty tree)."""
    import yaml
    with open(path) as f:
        return Reader(yaml.safe_load(f) or {})
