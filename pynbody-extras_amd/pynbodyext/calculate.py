"""Calculator layer: the call surface that drives the radial-profile path.

The reference's calculator DAG framework (pynbodyext/core/calculate/, ~7.6k
lines: engine, caching, tracing, pipelines) is out of scope (SURVEY.md §2
row 15); this module keeps the part of its API the hot path is reached
through, with the same names and semantics:

* ``CalculatorBase.__call__(sim, options=None, **overrides)`` -> value,
  ``run(...)`` -> :class:`Result`, ``filter(f)`` / ``with_filter(f)``
  (core/calculate/base.py:559-704),
* ``BoundCalculator``: evaluates its transform, then its filter scope in
  the transformed frame, then the wrapped calculator on ``source_sim[mask]``
  (base.py:874-1008, context.py:610-646); ``transform(t, revert=True)`` /
  ``with_transformation`` (template.py:39-58),
* ``FilterBase`` with ``&``, ``|``, ``~`` composition (filters.py:124-313),
* ``RunOptions`` / ``ExecutionContext.phase`` / dynamic parameters
  (context.py:503-533, base.py:422),
* ``PropertyBase`` with ``calculate(sim, params)``, the declarative
  ``PropertyBase.dataclass`` / ``Param`` fields and host-side arithmetic
  (``+ - * /``, unary ``-``) into ``OpProperty`` / ``ConstantProperty``
  (properties.py:125-295, fields.py:29-125, expr.py:117-260) and
  ``_in_sim_units`` (base.py:821-848); comparisons,
  ``clip``, caching, tracing and pipelines are not provided.

MI355X addition: a calculator may implement ``execute_fused(ctx, input,
filt)``; a bound calculator offers it its filter first, so a radial profile
behind a Sphere / FamilyFilter scope runs mask + r + binning as one device
pipeline instead of materialising the masked snapshot on the host.  A
transform scope does not rewrite ``pos`` / ``vel``: it resolves to a frame
(pynbodyext.frame) that rides along in those device passes, and the
snapshot an evaluation sees is a :class:`~pynbodyext.frame.FrameView`.
"""
from __future__ import annotations

import copy
import dataclasses
import operator
import threading
import time
from contextlib import contextmanager
from dataclasses import dataclass, field
from typing import Any

import numpy as np

__all__ = ["RunOptions", "Result", "NodeInput", "ExecutionContext", "CalculatorBase",
           "BoundCalculator", "FilterBase", "AndFilter", "OrFilter", "NotFilter",
           "resolve_value_in_units", "Param", "ParamView", "PropertyBase", "ConstantProperty",
           "OpProperty"]


BACKENDS = ("mi355x", "host")


@dataclass
class RunOptions:
    """backend: "mi355x" (default) lets a calculator take its device route;
    "host" keeps every calculator on the reference's numpy ``calculate`` /
    mask (profiles are built on the device either way).  A calculator
    evaluated from inside a run — a Sphere's radius given as a calculator —
    inherits the options of that run unless it is given its own."""

    cache: bool = True
    progress: Any = False
    perf_time: bool = False
    perf_memory: bool = False
    backend: str = "mi355x"
    default_record_policy: Any = None
    errors: str = "raise"
    cache_small_value_bytes: int = 0


@dataclass
class Result:
    value: Any
    perf: dict = field(default_factory=dict)

    def perf_summary(self) -> str:
        return ", ".join(f"{k}={v * 1e3:.2f} ms" for k, v in self.perf.items())


class NodeInput:
    """Snapshot view of one evaluation: the source snapshot and its selection."""

    def __init__(self, source_sim, mask=None, filt=None):
        self.source_sim = source_sim
        self.mask = mask
        self.filter = filt
        self._active = None

    @property
    def frame(self):
        """The frame ``source_sim`` is seen in (a FrameView's), or None."""
        return getattr(self.source_sim, "_frame", None)

    @property
    def active_sim(self):
        if self.mask is None:
            return self.source_sim
        if self._active is None:
            self._active = self.source_sim[np.asarray(self.mask, dtype=bool)]
        return self._active

    def with_selection(self, mask, filt=None) -> "NodeInput":
        if self.mask is not None:
            full = np.zeros(len(self.source_sim), dtype=bool)
            full[np.nonzero(self.mask)[0][np.asarray(mask, dtype=bool)]] = True
            mask = full
        return NodeInput(self.source_sim, mask, filt)


_active = threading.local()  # .stack: the ExecutionContexts of the runs in progress


class ExecutionContext:
    def __init__(self, options: RunOptions):
        if options.backend not in BACKENDS:
            raise ValueError(f"unknown backend {options.backend!r}; expected one of {list(BACKENDS)}")
        self.options = options
        self.perf: dict[str, float] = {}

    @property
    def on_host(self) -> bool:
        return self.options.backend == "host"

    @contextmanager
    def phase(self, node, name: str):
        t0 = time.perf_counter()
        try:
            yield
        finally:
            if self.options.perf_time:
                key = f"{type(node).__name__}.{name}"
                self.perf[key] = self.perf.get(key, 0.0) + time.perf_counter() - t0

    def raw_value(self, node: "CalculatorBase", input: NodeInput):
        return node.execute(self, input)

    def public_value(self, node: "CalculatorBase", input: NodeInput):
        return node.public_value(node.execute(self, input))


def resolve_value_in_units(value, sim, field_name: str | None):
    """Numbers pass through; unit strings / unit objects convert to the
    units of ``sim[field_name]``."""
    if value is None or isinstance(value, (int, float, np.floating, np.integer)):
        return value
    from ._pyn import units as _units

    if isinstance(value, str) or isinstance(value, getattr(_units, "UnitBase", ())):
        # (the unit table, not the array: a frame view derives its pos on demand)
        unit_of = getattr(sim, "_unit_of", None)
        target = None if not field_name else \
            unit_of(field_name) if unit_of is not None else sim[field_name].units
        u = _units.Unit(value) if isinstance(value, str) else value
        return float(u.ratio(target)) if target is not None else float(u.ratio(_units.NoUnit))
    return value


class CalculatorBase:
    """Base of every calculator node (reference core/calculate/base.py:209)."""

    dynamic_param_specs: dict[str, str | None] = {}
    default_options = RunOptions()

    # -- evaluation ------------------------------------------------------------
    def execute(self, ctx: ExecutionContext, input: NodeInput):
        raise NotImplementedError

    def public_value(self, value):
        return value

    def run(self, sim, options: RunOptions | None = None, **overrides) -> Result:
        stack = _active.__dict__.setdefault("stack", [])
        if options is not None:
            opts = copy.copy(options)
        else:  # (a run started from inside another inherits its options)
            opts = copy.copy(stack[-1].options if stack else self.default_options)
        for k, v in overrides.items():
            if v is not None:
                if not hasattr(opts, k):
                    raise TypeError(f"unknown run option {k!r}")
                setattr(opts, k, v)
        ctx = ExecutionContext(opts)
        stack.append(ctx)
        try:
            value = self.public_value(ctx.raw_value(self, NodeInput(sim)))
        finally:
            stack.pop()
            if stack:  # (its phases count in the run it was started from, too)
                outer = stack[-1].perf
                for k, v in ctx.perf.items():
                    outer[k] = outer.get(k, 0.0) + v
        return Result(value, ctx.perf)

    def __call__(self, sim, options: RunOptions | None = None, *, cache=None, progress=None,
                 perf_time=None, perf_memory=None, backend=None, default_record_policy=None,
                 errors=None, cache_small_value_bytes=None):
        return self.run(sim, options, cache=cache, progress=progress, perf_time=perf_time,
                        perf_memory=perf_memory, backend=backend,
                        default_record_policy=default_record_policy, errors=errors,
                        cache_small_value_bytes=cache_small_value_bytes).value

    def value(self, sim, options: RunOptions | None = None, **overrides):
        return self.run(sim, options, **overrides).value

    # -- scoping -----------------------------------------------------------------
    def with_filter(self, filt: "FilterBase") -> "BoundCalculator":
        return BoundCalculator(self, filt)

    def filter(self, filt: "FilterBase") -> "BoundCalculator":
        return self.with_filter(filt)

    def with_transformation(self, transform, *, revert: bool = True) -> "BoundCalculator":
        """This calculator evaluated in the frame ``transform`` (a
        pynbodyext.transforms node or chain) leads to.  revert=True leaves
        the snapshot as it was (it is never touched); revert=False rewrites
        its ``pos`` / ``vel`` into that frame once the value is computed."""
        return BoundCalculator(self, None, transform, revert)

    def transform(self, transform, *, revert: bool = True) -> "BoundCalculator":
        return self.with_transformation(transform, revert=revert)

    # -- dynamic parameters ------------------------------------------------------
    def resolve_dynamic_params(self, ctx: ExecutionContext, input: NodeInput) -> dict:
        out = {}
        sim = input.active_sim
        for name, field_name in self.dynamic_param_specs.items():
            v = getattr(self, name, None)
            if isinstance(v, CalculatorBase):
                v = ctx.public_value(v, input)
            elif callable(v):
                v = v(sim)
            out[name] = resolve_value_in_units(v, sim, field_name or "pos")
        return out

    def instance_signature(self):
        return (type(self).__name__, id(self))


class _Arithmetic:
    """Host-side ``+ - * /`` and unary ``-`` into OpProperty, shared by
    PropertyBase and BoundCalculator: a scoped property keeps them, as in
    ``0.5 * ParamContain("r").filter(f)``."""

    # -- host-side arithmetic --------------------------------------------------
    @classmethod
    def as_property(cls, other) -> "PropertyBase":
        return other if isinstance(other, CalculatorBase) else ConstantProperty(other)

    def __add__(self, other):
        return OpProperty("add", self, self.as_property(other))

    def __radd__(self, other):
        return OpProperty("add", self.as_property(other), self)

    def __sub__(self, other):
        return OpProperty("sub", self, self.as_property(other))

    def __rsub__(self, other):
        return OpProperty("sub", self.as_property(other), self)

    def __mul__(self, other):
        return OpProperty("mul", self, self.as_property(other))

    def __rmul__(self, other):
        return OpProperty("mul", self.as_property(other), self)

    def __truediv__(self, other):
        return OpProperty("truediv", self, self.as_property(other))

    def __rtruediv__(self, other):
        return OpProperty("truediv", self.as_property(other), self)

    def __neg__(self):
        return OpProperty("neg", self)


class BoundCalculator(_Arithmetic, CalculatorBase):
    """A calculator evaluated in a transform's frame (if any) on the subset
    selected by a filter scope (if any): the transform first, then the
    filter in the transformed frame, then the calculator."""

    def __init__(self, base: CalculatorBase, filt: "FilterBase | None" = None, transform=None,
                 revert: bool = True):
        self.base = base
        self.pre_filter = filt
        self.pre_transform = transform
        self.revert = bool(revert)

    def with_filter(self, filt: "FilterBase") -> "BoundCalculator":
        f = filt if self.pre_filter is None else self.pre_filter & filt
        return BoundCalculator(self.base, f, self.pre_transform, self.revert)

    def with_transformation(self, transform, *, revert: bool = True) -> "BoundCalculator":
        t = transform if self.pre_transform is None else self.pre_transform.then(transform)
        return BoundCalculator(self.base, self.pre_filter, t, self.revert and revert)

    def public_value(self, value):
        return self.base.public_value(value)

    def execute(self, ctx: ExecutionContext, input: NodeInput):
        if self.pre_transform is None:
            return self._execute_scoped(ctx, input)
        sim = input.active_sim
        with ctx.phase(self, "transform"):
            framed = self.pre_transform.framed_sim(ctx, sim)
        value = self._execute_scoped(ctx, NodeInput(framed))
        if not self.revert:
            with ctx.phase(self, "rewrite"):
                _rewrite_in_place(sim, framed)
        return value

    def _execute_scoped(self, ctx: ExecutionContext, input: NodeInput):
        if self.pre_filter is None:
            with ctx.phase(self, "calculate"):
                return ctx.raw_value(self.base, input)
        fused = getattr(self.base, "execute_fused", None)
        if fused is not None and input.mask is None and not ctx.on_host:
            with ctx.phase(self, "fused"):
                res = fused(ctx, input, self.pre_filter)
            if res is not NotImplemented:
                return res
        with ctx.phase(self, "filter"):
            mask = ctx.raw_value(self.pre_filter, input)
            work = input.with_selection(mask, self.pre_filter)
        with ctx.phase(self, "calculate"):
            return ctx.raw_value(self.base, work)


def _rewrite_in_place(sim, framed) -> None:
    """revert=False: the particles of ``sim`` take the positions and
    velocities ``framed`` (the same particles in the transform's frame)
    shows, written into the root snapshot's own arrays."""
    root = sim.ancestor
    index = getattr(sim, "_root_index", None)
    rows = slice(None) if index is None else index
    stored = getattr(root, "_arrays", None)
    for key in ("pos", "vel"):
        if stored is None:  # (a pynbody snapshot: its arrays write through)
            if key in root.keys():
                root[key][rows] = np.asarray(framed[key])
        elif key in stored:
            stored[key][rows] = np.asarray(framed[key])
    for s in (sim, root):
        getattr(s, "_derived", {}).clear()


class FilterBase(CalculatorBase):
    """Calculator producing a boolean mask over the active snapshot."""

    def build_mask(self, sim, params: dict) -> np.ndarray:
        raise NotImplementedError

    def execute(self, ctx: ExecutionContext, input: NodeInput) -> np.ndarray:
        sim = input.active_sim
        params = self.resolve_dynamic_params(ctx, input)
        return np.asarray(self.build_mask(sim, params), dtype=bool)

    def __call__(self, sim, *args, **kwargs):
        return self.value(sim)

    def device_spec(self, sim):
        """Device-fusable description ({"sphere": (cen, r), "families": [...],
        "region": [clauses of pynbodyext.region]}) or None when this filter
        cannot be fused."""
        return None

    def __and__(self, other: "FilterBase") -> "AndFilter":
        return AndFilter(self, other)

    def __or__(self, other: "FilterBase") -> "OrFilter":
        return OrFilter(self, other)

    def __invert__(self) -> "NotFilter":
        return NotFilter(self)


class AndFilter(FilterBase):
    def __init__(self, a: FilterBase, b: FilterBase):
        self.f1, self.f2 = a, b

    def execute(self, ctx, input):
        return ctx.raw_value(self.f1, input) & ctx.raw_value(self.f2, input)

    def device_spec(self, sim):
        return and_specs(self.f1.device_spec(sim), self.f2.device_spec(sim))


def and_specs(s1, s2):
    """The device_spec of the conjunction of two (None when either is, or
    when the region would exceed the library's clause limit).  The first
    Sphere keeps the sphere slot; a second one becomes a region clause."""
    from . import region as rg

    if s1 is None or s2 is None:
        return None
    out = {}
    clauses = list(s1.get("region") or ()) + list(s2.get("region") or ())
    sph = s1.get("sphere") or s2.get("sphere")
    if sph is not None:
        out["sphere"] = sph
    if "sphere" in s1 and "sphere" in s2:
        clauses.append(rg.sphere_clause(*s2["sphere"]))
    if len(clauses) > rg.REGION_MAX:
        return None
    if clauses:
        out["region"] = clauses
    f1, f2 = s1.get("families"), s2.get("families")
    if f1 is not None and f2 is not None:
        out["families"] = _intersect_ranges(f1, f2)
    elif f1 is not None or f2 is not None:
        out["families"] = f1 if f1 is not None else f2
    return out


class OrFilter(FilterBase):
    def __init__(self, a: FilterBase, b: FilterBase):
        self.f1, self.f2 = a, b

    def execute(self, ctx, input):
        return ctx.raw_value(self.f1, input) | ctx.raw_value(self.f2, input)

    def device_spec(self, sim):
        s1, s2 = self.f1.device_spec(sim), self.f2.device_spec(sim)
        # a union is fusable only between pure family selections
        if s1 is None or s2 is None or set(s1) != {"families"} or set(s2) != {"families"}:
            return None
        return {"families": sorted(s1["families"] + s2["families"])}


class NotFilter(FilterBase):
    def __init__(self, a: FilterBase):
        self.f = a

    def execute(self, ctx, input):
        return ~ctx.raw_value(self.f, input)

    def device_spec(self, sim):
        """The negated clause of a spec that is exactly one clause (a lone
        sphere or a one-clause region); anything else is not fusable."""
        from . import region as rg

        s = self.f.device_spec(sim)
        if s is None or len(s) != 1:
            return None
        if "sphere" in s:
            return {"region": [rg.sphere_clause(*s["sphere"], negate=True)]}
        if len(s.get("region") or ()) == 1:
            return {"region": [rg.negated(s["region"][0])]}
        return None


def _intersect_ranges(a, b):
    out = []
    for lo1, hi1 in a:
        for lo2, hi2 in b:
            lo, hi = max(lo1, lo2), min(hi1, hi2)
            if hi > lo:
                out.append((lo, hi))
    return out


# --------------------------------------------------------------------------
# properties
# --------------------------------------------------------------------------
class Param:
    """Marks a dynamic parameter of a declarative property
    (``frac: Param[float] = Param(default=0.5)``): a constant, a unit string
    (converted to the units of ``sim[field_name]``), a callable of the
    snapshot or another calculator, resolved when the property runs."""

    def __init__(self, default=dataclasses.MISSING, *, field_name: str | None = None):
        self.default = default
        self.field_name = field_name

    def __class_getitem__(cls, item):
        return cls


class ParamView:
    """The parameters ``calculate`` receives: the instance's fields with the
    dynamic ones resolved, by attribute or by item."""

    def __init__(self, values: dict):
        self.__dict__.update(values)

    def __getitem__(self, key):
        return self.__dict__[key]

    def __contains__(self, key):
        return key in self.__dict__

    def __repr__(self):
        return f"ParamView({self.__dict__!r})"


class PropertyBase(_Arithmetic, CalculatorBase):
    """Calculator reading one value from the active snapshot
    (reference core/calculate/properties.py:125).

    Subclasses implement ``calculate(sim, params=None)``.  MI355X addition: a
    property may implement ``device_plan(source, spec, params)``; on a root
    snapshot (unfiltered, or behind a filter scope the device understands) it
    then runs as one pass over the snapshot's arrays on the device instead
    of numpy passes over the masked sub-snapshot (pynbodyext/properties)."""

    def __class_getitem__(cls, item):
        return cls

    @classmethod
    def dataclass(cls, target=None, **dataclass_kwargs):
        """``dataclasses.dataclass`` for a property class; ``Param`` fields
        become ordinary fields with the Param's default and are recorded as
        dynamic parameters."""
        def wrap(t):
            specs = dict(getattr(t, "dynamic_param_specs", {}))
            for name, v in list(vars(t).items()):
                if isinstance(v, Param):
                    specs[name] = v.field_name
                    if v.default is dataclasses.MISSING:
                        delattr(t, name)
                    else:
                        setattr(t, name, v.default)
            t.dynamic_param_specs = specs
            dataclass_kwargs.setdefault("eq", False)  # identity hash, no truth-valued ==
            return dataclasses.dataclass(t, **dataclass_kwargs)

        return wrap if target is None else wrap(target)

    # -- evaluation ------------------------------------------------------------
    def calculate(self, sim, params=None):
        raise NotImplementedError(f"{type(self).__name__} must implement calculate()")

    def _params(self, ctx: ExecutionContext, input: NodeInput) -> ParamView:
        values = {}
        if dataclasses.is_dataclass(self):
            values = {f.name: getattr(self, f.name) for f in dataclasses.fields(self)}
        values.update(self.resolve_dynamic_params(ctx, input))
        return ParamView(values)

    def device_plan(self, source, spec: dict, params: ParamView):
        """A zero-argument callable evaluating this property on the device
        for the root snapshot ``source`` restricted by ``spec`` (a filter's
        ``device_spec``; {} = every particle), or None: no device route."""
        return None

    def _device_route(self, ctx: ExecutionContext, input: NodeInput, spec: dict):
        if type(self).device_plan is PropertyBase.device_plan or ctx.on_host:
            return NotImplemented
        # dynamic parameters are resolved on the snapshot the caller scoped:
        # one that depends on it keeps the two-step semantics behind a filter
        if spec and any(callable(getattr(self, k, None)) for k in self.dynamic_param_specs):
            return NotImplemented
        plan = self.device_plan(input.source_sim, spec, self._params(ctx, input))
        if plan is None:
            return NotImplemented
        with ctx.phase(self, "device"):
            return plan()

    def execute(self, ctx: ExecutionContext, input: NodeInput):
        if input.mask is None:
            res = self._device_route(ctx, input, {})
            if res is not NotImplemented:
                return res
        sim = input.active_sim
        params = self._params(ctx, input)
        with ctx.phase(self, "calculate"):
            return self.calculate(sim, params)

    def execute_fused(self, ctx: ExecutionContext, input: NodeInput, filt: "FilterBase"):
        spec = filt.device_spec(input.source_sim)
        if spec is None:
            return NotImplemented
        return self._device_route(ctx, input, spec)

    def _in_sim_units(self, value, sim_parameter: str, sim, target_units=None) -> float:
        """``value`` as a float in ``target_units`` (default: the units of
        ``sim[sim_parameter]``) — reference core/calculate/base.py:821-848.
        Numbers pass through, one-element arrays go through ``.item()``,
        ``SimArray`` and unit strings / objects are converted first."""
        from ._pyn import SimArray
        from ._pyn import units as _units

        target_unit = _units.Unit(target_units) if target_units is not None \
            else sim[sim_parameter].units
        context = sim.conversion_context() if hasattr(sim, "conversion_context") else {}
        if isinstance(value, str):
            value = _units.Unit(value)
        if isinstance(value, _units.UnitBase):
            value = float(value.in_units(target_unit, **context)) if hasattr(value, "in_units") \
                else float(value.ratio(target_unit))
        if isinstance(value, np.ndarray):
            if value.ndim == 0 or value.size == 1:
                if isinstance(value, SimArray):
                    value = value.in_units(target_unit, **context).item()
                else:
                    value = value.item()
            else:
                raise TypeError(f"value must be scalar-like, got shape {value.shape}")
        if isinstance(value, (int, float)):
            return float(value)
        raise TypeError(f"unsupported value type: {type(value)!r}")

    __hash__ = object.__hash__

    def __bool__(self) -> bool:
        raise TypeError("PropertyBase is symbolic; evaluate with run() or value().")


class ConstantProperty(PropertyBase):
    """A constant as a property (reference expr.py:117)."""

    def __init__(self, value):
        self.value_ = value

    def calculate(self, sim, params=None):
        return self.value_

    def __repr__(self):
        return f"ConstantProperty({self.value_!r})"


class OpProperty(PropertyBase):
    """``op`` applied on the host to the values of its operands, each
    evaluated on the same input (reference expr.py:199)."""

    _OPS = {"add": operator.add, "sub": operator.sub, "mul": operator.mul,
            "truediv": operator.truediv, "neg": operator.neg}

    def __init__(self, op_name: str, *operands: PropertyBase):
        if op_name not in self._OPS:
            raise ValueError(f"unknown operator {op_name!r}")
        self.op_name = op_name
        self.operands = operands

    def execute(self, ctx: ExecutionContext, input: NodeInput):
        values = [ctx.public_value(o, input) for o in self.operands]
        with ctx.phase(self, "calculate"):
            return self._OPS[self.op_name](*values)

    def __repr__(self):
        return f"OpProperty({self.op_name!r}, {', '.join(map(repr, self.operands))})"
