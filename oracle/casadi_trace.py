"""TEST-ONLY: a numeric stand-in for the small surface of CasADi that the reference's minimum-time NLP uses [REF opt_mintime_traj/src/opt_mintime.py]:
SX.sym, MX.sym, MX(ndarray), vertcat, Function, interpolant(.., 'linear', ..), collocation_points(3, 'legendre'), sin, cos, atan, exp, fmax, fmin,
dot, mtimes, sum1, nlpsol.  It solves nothing and differentiates nothing symbolically.  A symbolic scalar is a Node of a lazy expression graph; a
symbolic vector is a Vec of scalars (Nodes or numbers) with elementwise arithmetic, indexing and slicing.  evaluate() gives the graph numbers: a
binding of the leaf symbols and an Ops table that says what a constant, an arithmetic operation and the six functions mean for the scalar type --
float64, longdouble, a dual or a hyper-dual number, or Nodes again (that is how a Function substitutes its arguments).  Every node is evaluated
once (memoised by identity) on an explicit stack, so the objective's chain of N additions costs no recursion depth.

nlpsol() returns a Solver that records f, x, g and its call's x0, lbx, ubx, lbg, ubg, and answers with the point and multipliers injected through
configure(); its stats() say Solve_Succeeded.  oracle/mintime_trace.py puts this module into sys.modules as `casadi` around one run of the
reference's file.  Nothing of the reference is in here."""
import operator

import numpy as np

LD = np.longdouble
_BIN = {"add": operator.add, "sub": operator.sub, "mul": operator.mul, "div": operator.truediv}


class Node:
    """a scalar of the graph: op "sym" (a leaf), an arithmetic operation or a function, with Nodes or plain numbers as arguments"""
    __slots__ = ("op", "args", "name")
    __array_ufunc__ = None          # numpy_scalar * node reaches node.__rmul__
    __array_priority__ = 1000

    def __init__(self, op, args=(), name=None):
        self.op, self.args, self.name = op, tuple(args), name

    def __repr__(self):
        return self.name if self.op == "sym" else "<%s>" % self.op

    def __bool__(self):
        raise TypeError("casadi_trace: the truth value of a symbolic expression was asked for")

    def __add__(self, o):
        return _binary("add", self, o)

    def __radd__(self, o):
        return _binary("add", o, self)

    def __sub__(self, o):
        return _binary("sub", self, o)

    def __rsub__(self, o):
        return _binary("sub", o, self)

    def __mul__(self, o):
        return _binary("mul", self, o)

    def __rmul__(self, o):
        return _binary("mul", o, self)

    def __truediv__(self, o):
        return _binary("div", self, o)

    def __rtruediv__(self, o):
        return _binary("div", o, self)

    def __neg__(self):
        return Node("neg", (self,))

    def __pow__(self, p):
        """a whole power >= 1 as repeated products (the reference squares only)"""
        if isinstance(p, (Node, Vec)) or int(p) != p or p < 1:
            raise TypeError("casadi_trace: only whole powers >= 1 of an expression")
        out = self
        for _ in range(int(p) - 1):
            out = out * self
        return out


def _plural(x):
    return not isinstance(x, Node) and (isinstance(x, Vec) or (isinstance(x, (np.ndarray, list, tuple)) and np.ndim(x) > 0))


def _binary(op, a, b):
    if _plural(a) or _plural(b):
        return NotImplemented
    return Node(op, (a, b))


class Vec:
    """a column of scalars (Nodes or numbers): elementwise arithmetic with a scalar, a Vec, an array or a list of its length"""
    __array_ufunc__ = None
    __array_priority__ = 1000

    def __init__(self, items):
        self.items = list(items)

    def __len__(self):
        return len(self.items)

    def __iter__(self):
        return iter(self.items)

    @property
    def shape(self):
        return (len(self.items), 1)

    def __getitem__(self, i):
        if isinstance(i, slice):
            return Vec(self.items[i])
        return self.items[operator.index(i)]

    def _each(self, o, f):
        if isinstance(o, Vec):
            o = o.items
        elif _plural(o):
            o = list(np.ravel(o))
        else:
            o = [o] * len(self.items)
        if len(o) != len(self.items):
            raise ValueError("casadi_trace: %d against %d entries" % (len(self.items), len(o)))
        return Vec([f(a, b) for a, b in zip(self.items, o)])

    def __add__(self, o):
        return self._each(o, operator.add)
    __radd__ = __add__

    def __sub__(self, o):
        return self._each(o, operator.sub)

    def __rsub__(self, o):
        return self._each(o, lambda a, b: b - a)

    def __mul__(self, o):
        return self._each(o, operator.mul)

    def __rmul__(self, o):
        return self._each(o, lambda a, b: b * a)

    def __truediv__(self, o):
        return self._each(o, operator.truediv)

    def __rtruediv__(self, o):
        return self._each(o, lambda a, b: b / a)

    def __neg__(self):
        return Vec([-a for a in self.items])

    def __pow__(self, p):
        return Vec([a ** p for a in self.items])


def _symbolic(x):
    return isinstance(x, Node) or (isinstance(x, Vec) and any(isinstance(a, Node) for a in x.items))


def _sym(name, n=None):
    if n is None:
        return Node("sym", (), name)
    return Vec([Node("sym", (), "%s[%d]" % (name, i)) for i in range(int(n))])


class SX:
    sym = staticmethod(_sym)


class MX:
    """MX.sym as SX.sym; MX(array) is the array itself (mtimes and the operators take arrays)"""
    sym = staticmethod(_sym)

    def __new__(cls, a):
        return np.asarray(a)


def _items(x):
    if isinstance(x, Vec):
        return x.items
    if _plural(x):
        return list(np.ravel(x))
    return [x]


def vertcat(*parts):
    return Vec([a for p in parts for a in _items(p)])


def _function(name, f):
    def call(x):
        if isinstance(x, Vec):
            return Vec([call(a) for a in x.items])
        return Node(name, (x,)) if isinstance(x, Node) else f(x)
    return call


sin, cos, atan, exp = _function("sin", np.sin), _function("cos", np.cos), _function("atan", np.arctan), _function("exp", np.exp)


def fmax(a, b):
    return Node("fmax", (a, b)) if isinstance(a, Node) or isinstance(b, Node) else (a if a >= b else b)


def fmin(a, b):
    return Node("fmin", (a, b)) if isinstance(a, Node) or isinstance(b, Node) else (a if a <= b else b)


def _sum(terms):
    """from left to right"""
    acc = terms[0]
    for t in terms[1:]:
        acc = acc + t
    return acc


def dot(a, b):
    a, b = _items(a), _items(b)
    if len(a) != len(b):
        raise ValueError("casadi_trace: dot of %d and %d entries" % (len(a), len(b)))
    return _sum([x * y for x, y in zip(a, b)])


def sum1(x):
    return _sum(_items(x))


def mtimes(A, x):
    """a numeric matrix times a column; the products with an exact zero of the matrix are left out (they add nothing to a finite sum)"""
    A, x = np.asarray(A), _items(x)
    if A.ndim != 2 or A.shape[1] != len(x):
        raise ValueError("casadi_trace: mtimes of %s and %d entries" % (A.shape, len(x)))
    rows = []
    for r in A:
        terms = [r[j] * x[j] for j in range(len(x)) if r[j] != 0]
        rows.append(_sum(terms) if terms else 0.0)
    return Vec(rows)


class Ops:
    """what the graph's operations mean for one scalar type: const lifts a plain number, value gives the number that fmax / fmin branch on"""

    def __init__(self, const, sin, cos, atan, exp, value=lambda x: x):
        self.const, self.value = const, value
        self.fn = {"sin": sin, "cos": cos, "atan": atan, "exp": exp}

    def apply(self, op, v):
        if op in _BIN:
            return _BIN[op](v[0], v[1])
        if op == "neg":
            return -v[0]
        if op == "fmax":
            return v[0] if self.value(v[0]) >= self.value(v[1]) else v[1]
        if op == "fmin":
            return v[0] if self.value(v[0]) <= self.value(v[1]) else v[1]
        return self.fn[op](v[0])


class _Substitute(Ops):
    """Nodes for Nodes: the module's own functions rebuild the graph (and fold what has become numeric)"""

    def __init__(self):
        Ops.__init__(self, lambda c: c, sin, cos, atan, exp)

    def apply(self, op, v):
        if op == "fmax":
            return fmax(v[0], v[1])
        if op == "fmin":
            return fmin(v[0], v[1])
        return Ops.apply(self, op, v)


def number_ops(dtype):
    return Ops(dtype, np.sin, np.cos, np.arctan, np.exp)


def evaluate(outputs, binding, ops):
    """The values of a list of scalars (Nodes or numbers).  binding: {id(leaf): value of the scalar type}.  Every node once, no recursion."""
    memo = dict(binding)
    stack = [o for o in outputs if isinstance(o, Node)]
    while stack:
        n = stack[-1]
        if id(n) in memo:
            stack.pop()
            continue
        pending = [a for a in n.args if isinstance(a, Node) and id(a) not in memo]
        if pending:
            stack.extend(pending)
            continue
        stack.pop()
        if n.op == "sym":
            raise KeyError("casadi_trace: the symbol %s is not bound" % n.name)
        memo[id(n)] = ops.apply(n.op, [memo[id(a)] if isinstance(a, Node) else ops.const(a) for a in n.args])
    return [memo[id(o)] if isinstance(o, Node) else ops.const(o) for o in outputs]


def count_nodes(outputs):
    seen, stack = set(), [o for o in outputs if isinstance(o, Node)]
    while stack:
        n = stack.pop()
        if id(n) not in seen:
            seen.add(id(n))
            stack.extend(a for a in n.args if isinstance(a, Node))
    return len(seen)


class Function:
    """Function(name, ins, outs, ...): called with expressions it substitutes them, called with numbers it evaluates in the configured dtype.
    One output comes back bare, several as a list; a vector output is a Vec (symbolic) or a 1-D array (numeric)."""

    def __init__(self, name, ins, outs, *names):
        self.name, self.ins, self.outs = name, list(ins), list(outs)
        _STATE["functions"][name] = self

    def bind(self, args, lift=lambda a: a):
        if len(args) != len(self.ins):
            raise TypeError("casadi_trace: %s takes %d arguments" % (self.name, len(self.ins)))
        binding = {}
        for s, a in zip(self.ins, args):
            ss, aa = _items(s), _items(a)
            if len(ss) != len(aa):
                raise ValueError("casadi_trace: %s: an argument of %d entries for %d" % (self.name, len(aa), len(ss)))
            binding.update((id(x), lift(y)) for x, y in zip(ss, aa))
        return binding

    def eval(self, args, ops, lift=None):
        """the outputs as lists of scalars of ops' type"""
        flat = [a for o in self.outs for a in _items(o)]
        vals = evaluate(flat, self.bind(args, ops.const if lift is None else lift), ops)
        out, at = [], 0
        for o in self.outs:
            n = len(_items(o))
            out.append((vals[at:at + n], isinstance(o, Vec)))
            at += n
        return out

    def __call__(self, *args):
        if any(_symbolic(a) for a in args):
            res = [Vec(v) if is_vec else v[0] for v, is_vec in self.eval(args, _Substitute(), lambda a: a)]
        else:
            dtype = _STATE["dtype"]
            res = [np.array(v, dtype=dtype) if is_vec else v[0] for v, is_vec in self.eval(args, number_ops(dtype))]
        return res[0] if len(res) == 1 else res


def interpolant(name, kind, grid, values):
    """the piecewise-linear function of the step index: a whole index returns the sample itself as a plain float64"""
    if kind != "linear" or len(grid) != 1:
        raise NotImplementedError("casadi_trace: interpolant %r on %d grids" % (kind, len(grid)))
    steps, vals = np.asarray(grid[0], dtype=np.float64), np.asarray(values, dtype=np.float64)
    if steps.shape != vals.shape or not np.array_equal(steps, np.arange(steps.size)):
        raise NotImplementedError("casadi_trace: the interpolant's grid must be 0, 1, .., n - 1")

    def f(x):
        if isinstance(x, (Node, Vec)):
            raise NotImplementedError("casadi_trace: an interpolant of an expression")
        i = int(np.floor(x))
        if x == i:
            return np.float64(vals[i])
        t = type(x) if isinstance(x, np.floating) else np.float64
        return t(vals[i]) + (x - i) * (t(vals[i + 1]) - t(vals[i]))
    return f


def collocation_points(d, scheme):
    """the Gauss-Legendre points of degree 3 on (0, 1): computed in longdouble, returned in the configured dtype"""
    if d != 3 or scheme != "legendre":
        raise NotImplementedError("casadi_trace: collocation_points(%r, %r)" % (d, scheme))
    s = np.sqrt(LD(15)) / LD(10)
    return np.array([LD(0.5) - s, LD(0.5), LD(0.5) + s], dtype=LD).astype(_STATE["dtype"])


class Solver:
    def __init__(self, name, plugin, nlp, opts):
        self.name, self.plugin, self.opts = name, plugin, dict(opts)
        self.f, self.x, self.g = nlp["f"], nlp["x"], nlp["g"]
        self.call = None

    def __call__(self, **kw):
        self.call = {k: np.array(v) for k, v in kw.items()}
        inj, dtype = _STATE["inject"], _STATE["dtype"]
        if len(inj["x"]) != len(self.x):
            raise ValueError("casadi_trace: the injected point holds %d entries, the NLP %d" % (len(inj["x"]), len(self.x)))
        return {k: np.asarray(inj[k], dtype=np.float64).astype(dtype) for k in ("x", "lam_x", "lam_g")}

    def stats(self):
        return {"return_status": "Solve_Succeeded", "success": True}


def nlpsol(name, plugin, nlp, opts=None):
    s = Solver(name, plugin, nlp, opts or {})
    _STATE["solvers"].append(s)
    return s


_STATE = dict(dtype=np.float64, inject=None, functions={}, solvers=[])


def configure(dtype, x, lam_x, lam_g):
    """A fresh record: the dtype numeric calls answer in, and what the solver returns."""
    _STATE.update(dtype=dtype, inject=dict(x=x, lam_x=lam_x, lam_g=lam_g), functions={}, solvers=[])


def record():
    """(the one Solver of the run, {name: Function})"""
    if len(_STATE["solvers"]) != 1:
        raise RuntimeError("casadi_trace: %d nlpsol calls recorded" % len(_STATE["solvers"]))
    return _STATE["solvers"][0], dict(_STATE["functions"])
