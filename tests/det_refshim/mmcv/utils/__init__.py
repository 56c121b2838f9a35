"""mmcv.utils.Registry, reduced to register_module() / build(cfg) with parent lookup."""


class Registry:
    def __init__(self, name, parent=None):
        self.name, self.parent, self._modules = name, parent, {}

    def register_module(self, name=None, module=None):
        def deco(cls):
            self._modules[name or cls.__name__] = cls
            return cls
        return deco(module) if module is not None else deco

    def get(self, key):
        if key in self._modules:
            return self._modules[key]
        return self.parent.get(key) if self.parent is not None else None

    def build(self, cfg):
        cfg = dict(cfg)
        cls = self.get(cfg.pop('type'))
        return cls(**cfg)
