"""Self-hosted plugin surface: a minimal Registry with the build-from-config-dict semantics the
reference relies on (mmengine.Registry is not installed here nor assumed on the GPU box).

Mirrors reference mmtrack/registry.py:33-77 (MODELS, TASK_UTILS, ... as children of the mmengine
roots) for the registries the hot path touches.  `type` strings may carry a scope prefix
('mmtrack.X', 'mmdet.X', 'mmyolo.X') or the dict may carry `_scope_`; both are accepted and
resolved against the same table, so config files shaped like
configs/stereo_tracking/ocsort/yolox_s_mmyolo_mot_airdrone_disp.py build unchanged.
If mmengine IS importable, classes are additionally registered into its MODELS / TASK_UTILS roots.
"""
import inspect

_KNOWN_SCOPES = ('mmtrack', 'mmdet', 'mmyolo', 'mmengine', 'mmcv', 'stereotracking_amd')


class Registry:
    def __init__(self, name, parent=None):
        self.name = name
        self.parent = parent
        self._modules = {}

    def register_module(self, name=None, force=False, module=None):
        def _register(cls):
            names = [name] if isinstance(name, str) else (name or [cls.__name__])
            for n in names:
                if n in self._modules and not force and self._modules[n] is not cls:
                    raise KeyError(f'{n} is already registered in {self.name}')
                self._modules[n] = cls
            return cls
        if module is not None:
            return _register(module)
        return _register

    def get(self, key):
        if '.' in key:
            scope, _, rest = key.partition('.')
            if scope in _KNOWN_SCOPES:
                key = rest
        if key in self._modules:
            return self._modules[key]
        if self.parent is not None:
            return self.parent.get(key)
        return None

    def build(self, cfg, *args, **kwargs):
        if cfg is None:
            return None
        if not isinstance(cfg, dict):
            raise TypeError(f'cfg must be a dict, got {type(cfg)}')
        if 'type' not in cfg:
            raise KeyError(f'`cfg` must contain the key "type", but got {cfg}')
        cfg = dict(cfg)
        cfg.pop('_scope_', None)
        obj_type = cfg.pop('type')
        if isinstance(obj_type, str):
            obj_cls = self.get(obj_type)
            if obj_cls is None:
                raise KeyError(f'{obj_type} is not in the {self.name} registry')
        elif inspect.isclass(obj_type) or callable(obj_type):
            obj_cls = obj_type
        else:
            raise TypeError(f'type must be a str or class, got {type(obj_type)}')
        return obj_cls(*args, **cfg, **kwargs)

    def __contains__(self, key):
        return self.get(key) is not None

    def __repr__(self):
        return f'Registry(name={self.name}, items={sorted(self._modules)})'


MODELS = Registry('model')
TASK_UTILS = Registry('task util')
TRANSFORMS = Registry('transform')
DATASETS = Registry('dataset')
DATA_SAMPLERS = Registry('data sampler')
METRICS = Registry('metric')
VISUALIZERS = Registry('visualizer')
HOOKS = Registry('hook')


def mirror_into_mmengine():
    """Best effort: expose the same classes through mmengine's registries when it is installed."""
    try:
        from mmengine.registry import MODELS as MM_MODELS, TASK_UTILS as MM_TASK_UTILS
    except Exception:  # noqa: BLE001 - mmengine absent is the normal case here
        return False
    for src, dst in ((MODELS, MM_MODELS), (TASK_UTILS, MM_TASK_UTILS)):
        for n, cls in src._modules.items():
            try:
                dst.register_module(name=n, module=cls, force=True)
            except Exception:  # noqa: BLE001
                pass
    return True
