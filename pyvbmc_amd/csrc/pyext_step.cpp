// The repeat path of _neg_elcbo as a CPython type (pyvbmc_amd/variational_optimization.py, _FastElbo).
//
// Between two evaluations of a polled step the device is idle while the host turns round: return from the C call,
// build the result, the caller, re-entry, the re-checks, pack theta, call again.  FastElboBase.call is
// _FastElbo._call_py statement for statement -- the same attribute reads, the same comparisons with the same outcomes,
// in the same order -- without the interpreter.  Anything that is not the plain repeat (a theta that is not an aligned
// contiguous float64 vector of the right length, a seed that is not an int, a return code, side effects the release
// callback did not get to apply) goes to the Python methods `_call_py` / `_finish_py` of the subclass, so those paths
// keep one implementation.  Host C++ only; no device code.
#define PY_SSIZE_T_CLEAN
#include <Python.h>
#include <structmember.h>

#define NPY_NO_DEPRECATED_API NPY_1_7_API_VERSION
#include <numpy/arrayobject.h>

#include "step_lane.h"

namespace {

struct FastElbo {
  PyObject_HEAD
  // what _FastElbo holds (its former __slots__), readable and writable from Python under the same names
  PyObject *ctx_arg, *ctx, *fc, *vp, *gp, *bnd, *Ns, *cg, *rng, *mask, *D, *K, *n_theta, *philox, *lb, *ub, *tol, *wthr,
      *wpen, *fused_last;
  PyObject* keep;  // owners of the memory `lane` points into
  StepLane lane;
};

#define FE_OBJECTS(X)                                                                                                  \
  X(ctx_arg) X(ctx) X(fc) X(vp) X(gp) X(bnd) X(Ns) X(cg) X(rng) X(mask) X(D) X(K) X(n_theta) X(philox) X(lb) X(ub)    \
  X(tol) X(wthr) X(wpen) X(fused_last)

// set once by setup(): the module globals of variational_optimization (for _FAST_PATH, read at call time), ctx_of,
// philox_seed
PyObject *g_globals, *g_lib_globals, *g_ctx_of, *g_philox_seed, *s_default_ctx;
PyObject *s_FAST_PATH, *s_optimize_mu, *s_optimize_sigma, *s_optimize_lambd, *s_optimize_weights, *s_D, *s_K, *s_dict,
    *s_fused_last, *s_ctx, *s_lb, *s_ub, *s_tol_con, *s_weight_threshold, *s_weight_penalty, *s_get, *s_posteriors, *s_X,
    *s_shape, *s_gp_quick, *s_alpha, *s_hyp, *s_side, *s_call_py, *s_finish_py, *g_zero_f, *g_zero_i;

// `a != b` as the interpreter evaluates it (no identity short cut: nan != nan also for one object)
int ne(PyObject* a, PyObject* b) {
  if (PyFloat_CheckExact(a) && PyFloat_CheckExact(b)) return PyFloat_AS_DOUBLE(a) != PyFloat_AS_DOUBLE(b);
  PyObject* r = PyObject_RichCompare(a, b, Py_NE);
  if (!r) return -1;
  const int t = PyObject_IsTrue(r);
  Py_DECREF(r);
  return t;
}

// `v != obj` for a C long v
int ne_long(long v, PyObject* obj) {
  if (PyLong_CheckExact(obj)) {
    int ovf = 0;
    const long o = PyLong_AsLongAndOverflow(obj, &ovf);
    return ovf ? 1 : o != v;
  }
  PyObject* pv = PyLong_FromLong(v);
  if (!pv) return -1;
  const int t = ne(pv, obj);
  Py_DECREF(pv);
  return t;
}

// getattr(o, name, None)
PyObject* getattr_or_none(PyObject* o, PyObject* name) {
  PyObject* r = PyObject_GetAttr(o, name);
  if (!r && PyErr_ExceptionMatches(PyExc_AttributeError)) {
    PyErr_Clear();
    r = Py_None;
    Py_INCREF(r);
  }
  return r;
}

// m.get(key, dflt) -> new reference
PyObject* map_get(PyObject* m, PyObject* key, PyObject* dflt) {
  if (PyDict_CheckExact(m)) {
    PyObject* r = PyDict_GetItemWithError(m, key);
    if (!r) {
      if (PyErr_Occurred()) return nullptr;
      r = dflt;
    }
    Py_INCREF(r);
    return r;
  }
  return PyObject_CallMethodObjArgs(m, s_get, key, dflt, nullptr);
}

// o.__dict__.get(key) -> new reference
PyObject* dict_attr_get(PyObject* o, PyObject* key) {
  PyObject* d = PyObject_GetAttr(o, s_dict);
  if (!d) return nullptr;
  PyObject* r = map_get(d, key, Py_None);
  Py_DECREF(d);
  return r;
}

// 1 / 0 / -1: bool(getattr(o, name))
int attr_true(PyObject* o, PyObject* name) {
  PyObject* v = PyObject_GetAttr(o, name);
  if (!v) return -1;
  const int t = PyObject_IsTrue(v);
  Py_DECREF(v);
  return t;
}

// getattr(o, name) != want
int attr_ne(PyObject* o, PyObject* name, PyObject* want) {
  PyObject* v = PyObject_GetAttr(o, name);
  if (!v) return -1;
  const int t = ne(v, want);
  Py_DECREF(v);
  return t;
}

// One entry of the `quick` list the Python statement forms: id(object) or a value (X.shape[0])
struct QuickItem {
  void* id;
  PyObject* value;  // borrowed, alive for the comparison; nullptr: an id entry
};

// item == what the stored list holds there (the list comparison's identity short cut included)
int quick_item_equal(const QuickItem& it, PyObject* stored) {
  if (it.value) return PyObject_RichCompareBool(it.value, stored, Py_EQ);
  if (PyLong_CheckExact(stored)) {
    void* p = PyLong_AsVoidPtr(stored);
    if (!p && PyErr_Occurred()) {
      PyErr_Clear();
      return 0;
    }
    return p == it.id;
  }
  PyObject* v = PyLong_FromVoidPtr(it.id);
  if (!v) return -1;
  const int e = PyObject_RichCompareBool(v, stored, Py_EQ);
  Py_DECREF(v);
  return e;
}

// quick = [id(ps), id(X), X.shape[0]] + [id(p), id(p.alpha), id(p.hyp) for p in ps];
// quick != ctx.__dict__.get("_gp_quick"): 1 differs, 0 equal, -1 error
int gp_quick_differs(PyObject* gp, PyObject* ctx) {
  PyObject *ps = nullptr, *X = nullptr, *shape = nullptr, *n0 = nullptr, *stored = nullptr, *it = nullptr;
  QuickItem small[3 + 3 * 8];
  QuickItem* items = small;
  Py_ssize_t n = 0, cap = sizeof(small) / sizeof(small[0]);
  int out = -1;
  do {
    if (!(ps = PyObject_GetAttr(gp, s_posteriors))) break;
    if (!(X = PyObject_GetAttr(gp, s_X))) break;
    if (!(shape = PyObject_GetAttr(X, s_shape))) break;
    if (!(n0 = PySequence_GetItem(shape, 0))) break;
    items[n++] = {ps, nullptr};
    items[n++] = {X, nullptr};
    items[n++] = {nullptr, n0};
    if (!(it = PyObject_GetIter(ps))) break;
    bool bad = false;
    while (PyObject* p = PyIter_Next(it)) {
      if (n + 3 > cap) {
        QuickItem* grown = static_cast<QuickItem*>(PyMem_Malloc(sizeof(QuickItem) * 2 * cap));
        if (!grown) {
          PyErr_NoMemory();
          Py_DECREF(p);
          bad = true;
          break;
        }
        for (Py_ssize_t i = 0; i < n; ++i) grown[i] = items[i];
        if (items != small) PyMem_Free(items);
        items = grown;
        cap *= 2;
      }
      // (ids of attribute values that may be temporaries, as id(p.alpha) is)
      PyObject* a = PyObject_GetAttr(p, s_alpha);
      PyObject* h = a ? PyObject_GetAttr(p, s_hyp) : nullptr;
      items[n++] = {p, nullptr};
      items[n++] = {a, nullptr};
      items[n++] = {h, nullptr};
      Py_XDECREF(h);
      Py_XDECREF(a);
      Py_DECREF(p);
      if (!a || !h) {
        bad = true;
        break;
      }
    }
    if (bad || PyErr_Occurred()) break;
    if (!(stored = dict_attr_get(ctx, s_gp_quick))) break;
    if (!PyList_Check(stored) || PyList_GET_SIZE(stored) != n) {
      out = 1;
      break;
    }
    out = 0;
    for (Py_ssize_t i = 0; i < n && out == 0; ++i) {
      if (i >= PyList_GET_SIZE(stored)) {  // (an __eq__ that shortened the list)
        out = 1;
        break;
      }
      PyObject* si = PyList_GET_ITEM(stored, i);
      Py_INCREF(si);
      const int e = quick_item_equal(items[i], si);
      Py_DECREF(si);
      out = e < 0 ? -1 : !e;
    }
  } while (false);
  if (items != small) PyMem_Free(items);
  Py_XDECREF(it);
  Py_XDECREF(stored);
  Py_XDECREF(n0);
  Py_XDECREF(shape);
  Py_XDECREF(X);
  Py_XDECREF(ps);
  return out;
}

// ctx_of(vp, ctx_arg): the explicit one, the one vp was given, or (through the Python function) the process-wide default
PyObject* ctx_of(PyObject* vp, PyObject* ctx_arg) {
  if (ctx_arg != Py_None) {
    Py_INCREF(ctx_arg);
    return ctx_arg;
  }
  PyObject* own = getattr_or_none(vp, s_ctx);
  if (!own || own != Py_None) return own;
  Py_DECREF(own);
  // _lib.default_context() while a default exists; creating one is the Python function's
  PyObject* dflt = PyDict_GetItemWithError(g_lib_globals, s_default_ctx);
  if (dflt && dflt != Py_None) {
    Py_INCREF(dflt);
    return dflt;
  }
  if (!dflt && PyErr_Occurred()) return nullptr;
  return PyObject_CallFunctionObjArgs(g_ctx_of, vp, ctx_arg, nullptr);
}

bool plain_vector(PyObject* theta, int64_t n) {
  if (!PyArray_CheckExact(theta)) return false;
  PyArrayObject* a = reinterpret_cast<PyArrayObject*>(theta);
  return PyArray_TYPE(a) == NPY_DOUBLE && PyArray_ISNOTSWAPPED(a) && PyArray_NDIM(a) == 1 && PyArray_DIM(a, 0) == n &&
         PyArray_IS_C_CONTIGUOUS(a) && PyArray_ISALIGNED(a);
}

PyObject* fe_call(PyObject* self_, PyObject* const* args, Py_ssize_t nargs) {
  FastElbo* s = reinterpret_cast<FastElbo*>(self_);
  if (nargs != 2) {
    PyErr_SetString(PyExc_TypeError, "call(theta, seed)");
    return nullptr;
  }
  PyObject *theta = args[0], *seed = args[1];
  // not the plain repeat: the Python statement of the same method
  if (!s->lane.fn || !plain_vector(theta, s->lane.n_theta) || !(seed == Py_None || PyLong_CheckExact(seed)))
    return PyObject_CallMethodObjArgs(self_, s_call_py, theta, seed, nullptr);
#define NEED(f)                                                \
  if (!s->f) {                                                 \
    PyErr_SetString(PyExc_AttributeError, #f);                 \
    return nullptr;                                            \
  }
  NEED(vp) NEED(ctx) NEED(fc) NEED(bnd) NEED(mask) NEED(D) NEED(K) NEED(fused_last) NEED(ctx_arg) NEED(gp) NEED(philox)
  NEED(cg)
#undef NEED
  PyObject* fp = PyDict_GetItemWithError(g_globals, s_FAST_PATH);
  if (!fp) {
    if (!PyErr_Occurred()) PyErr_SetString(PyExc_NameError, "name '_FAST_PATH' is not defined");
    return nullptr;
  }
  int t = PyObject_IsTrue(fp);
  if (t < 0) return nullptr;
  if (!t) Py_RETURN_NONE;
  PyObject *vp = s->vp, *ctx = s->ctx, *fc = s->fc, *bnd = s->bnd;
#define TRY(expr)            \
  if ((t = (expr)) < 0) return nullptr;
#define NONE_IF(expr)        \
  TRY(expr)                  \
  if (t) Py_RETURN_NONE;
  long mask = 0;
  TRY(attr_true(vp, s_optimize_mu)) mask |= t ? 1 : 0;
  TRY(attr_true(vp, s_optimize_sigma)) mask |= t ? 2 : 0;
  TRY(attr_true(vp, s_optimize_lambd)) mask |= t ? 4 : 0;
  TRY(attr_true(vp, s_optimize_weights)) mask |= t ? 8 : 0;
  NONE_IF(ne_long(mask, s->mask))
  NONE_IF(attr_ne(vp, s_D, s->D))
  NONE_IF(attr_ne(vp, s_K, s->K))
  {
    PyObject* fl = dict_attr_get(ctx, s_fused_last);
    if (!fl) return nullptr;
    const bool same = fl == s->fused_last;
    Py_DECREF(fl);
    if (!same) Py_RETURN_NONE;
    PyObject* v = getattr_or_none(ctx, s_D);
    if (!v) return nullptr;
    t = ne(v, s->D);
    Py_DECREF(v);
    NONE_IF(t)
    if (!(v = getattr_or_none(ctx, s_K))) return nullptr;
    t = ne(v, s->K);
    Py_DECREF(v);
    NONE_IF(t)
    if (!(v = ctx_of(vp, s->ctx_arg))) return nullptr;
    const bool is_ctx = v == ctx;
    Py_DECREF(v);
    if (!is_ctx) Py_RETURN_NONE;
  }
  NONE_IF(ne_long(15, s->mask))
  if (bnd != Py_None) {
    PyObject* v = PyObject_GetItem(bnd, s_lb);
    if (!v) return nullptr;
    bool other = v != s->lb;
    Py_DECREF(v);
    if (other) Py_RETURN_NONE;
    if (!(v = PyObject_GetItem(bnd, s_ub))) return nullptr;
    other = v != s->ub;
    Py_DECREF(v);
    if (other) Py_RETURN_NONE;
    if (!s->tol || !s->wthr || !s->wpen) {
      PyErr_SetString(PyExc_AttributeError, "tol");
      return nullptr;
    }
    if (!(v = PyObject_GetItem(bnd, s_tol_con))) return nullptr;
    t = ne(v, s->tol);
    Py_DECREF(v);
    NONE_IF(t)
    if (!(v = map_get(bnd, s_weight_threshold, g_zero_f))) return nullptr;
    t = ne(v, s->wthr);
    Py_DECREF(v);
    NONE_IF(t)
    if (!(v = map_get(bnd, s_weight_penalty, g_zero_f))) return nullptr;
    t = ne(v, s->wpen);
    Py_DECREF(v);
    NONE_IF(t)
  }
  NONE_IF(gp_quick_differs(s->gp, ctx))
  // fc.th[:] = theta
  step_lane_pack(s->lane, static_cast<const double*>(PyArray_DATA(reinterpret_cast<PyArrayObject*>(theta))));
  TRY(PyObject_IsTrue(s->cg))
  const int cg = t;
  TRY(PyObject_IsTrue(s->philox))
  if (t) {
    if (seed == Py_None) {
      PyObject* sd = PyObject_CallFunctionObjArgs(g_philox_seed, ctx, nullptr);
      if (!sd) return nullptr;
      const unsigned long long v = PyLong_AsUnsignedLongLongMask(sd);
      Py_DECREF(sd);
      if (v == static_cast<unsigned long long>(-1) && PyErr_Occurred()) return nullptr;
      *s->lane.seed = v;
    } else {
      const unsigned long long v = PyLong_AsUnsignedLongLongMask(seed);  // (as a ctypes c_uint64 field takes an int)
      if (v == static_cast<unsigned long long>(-1) && PyErr_Occurred()) return nullptr;
      *s->lane.seed = v;
    }
  }
  // fc.side = (vp, theta, self.mask, self.K)
  {
    PyObject* side = PyTuple_Pack(4, vp, theta, s->mask, s->K);
    if (!side) return nullptr;
    const int rc = PyObject_SetAttr(fc, s_side, side);
    Py_DECREF(side);
    if (rc < 0) return nullptr;
  }
  const StepLane lane = s->lane;  // (held across the call: the callback runs Python code)
  Py_INCREF(self_);
  Py_INCREF(fc);
  int rc;
  Py_BEGIN_ALLOW_THREADS
  rc = step_lane_invoke(lane);
  Py_END_ALLOW_THREADS
  PyObject* out = nullptr;
  do {
    if (PyErr_Occurred()) {  // try / finally: fc.side = None, the exception goes on
      PyObject *et, *ev, *tb;
      PyErr_Fetch(&et, &ev, &tb);
      if (PyObject_SetAttr(fc, s_side, Py_None) < 0) PyErr_Clear();
      PyErr_Restore(et, ev, tb);
      break;
    }
    PyObject* side = PyObject_GetAttr(fc, s_side);
    if (!side) break;
    const bool applied = side == Py_None;
    Py_DECREF(side);
    if (rc != 0 || !applied) {
      // a return code (W_GP_CHANGED among them) or side effects still to be applied: the Python statement from
      // the point after the C call
      PyObject* prc = PyLong_FromLong(rc);
      if (!prc) break;
      out = PyObject_CallMethodObjArgs(self_, s_finish_py, prc, nullptr);
      Py_DECREF(prc);
      break;
    }
    PyObject *F = PyFloat_FromDouble(*lane.F), *G = PyFloat_FromDouble(*lane.G), *H = PyFloat_FromDouble(*lane.H);
    PyObject* dF = nullptr;
    if (cg) {
      npy_intp n = static_cast<npy_intp>(lane.n_theta);
      dF = PyArray_SimpleNew(1, &n, NPY_DOUBLE);
      if (dF) step_lane_grad(lane, static_cast<double*>(PyArray_DATA(reinterpret_cast<PyArrayObject*>(dF))));
    } else {
      dF = Py_None;
      Py_INCREF(dF);
    }
    if (F && G && H && dF) out = PyTuple_Pack(5, F, dF, G, H, g_zero_i);
    Py_XDECREF(F);
    Py_XDECREF(G);
    Py_XDECREF(H);
    Py_XDECREF(dF);
  } while (false);
  Py_DECREF(fc);
  Py_DECREF(self_);
  return out;
#undef TRY
#undef NONE_IF
}

// _bind_lane(fn, handle, block, th, dF, F, G, H, seed, keep): addresses as ints; th / dF the block's float64 vectors
PyObject* fe_bind(PyObject* self_, PyObject* args) {
  FastElbo* s = reinterpret_cast<FastElbo*>(self_);
  unsigned long long fn, handle, block, F, G, H, seed;
  PyObject *th, *dF, *keep;
  if (!PyArg_ParseTuple(args, "KKKOOKKKKO", &fn, &handle, &block, &th, &dF, &F, &G, &H, &seed, &keep)) return nullptr;
  if (!PyArray_CheckExact(th) || !PyArray_CheckExact(dF)) {
    PyErr_SetString(PyExc_TypeError, "th and dF must be ndarrays");
    return nullptr;
  }
  PyArrayObject *a = reinterpret_cast<PyArrayObject*>(th), *b = reinterpret_cast<PyArrayObject*>(dF);
  if (PyArray_NDIM(a) != 1 || !plain_vector(dF, PyArray_DIM(a, 0)) || !plain_vector(th, PyArray_DIM(a, 0)) ||
      !PyArray_ISWRITEABLE(a) || !fn || !block || !F || !G || !H || !seed) {
    PyErr_SetString(PyExc_ValueError, "the argument block's theta and dF must be float64 vectors of one length");
    return nullptr;
  }
  PyObject* held = PyTuple_Pack(3, th, dF, keep);
  if (!held) return nullptr;
  Py_XSETREF(s->keep, held);
  StepLane& l = s->lane;
  l.fn = reinterpret_cast<int (*)(void*, const void*)>(static_cast<uintptr_t>(fn));
  l.handle = reinterpret_cast<void*>(static_cast<uintptr_t>(handle));
  l.block = reinterpret_cast<const void*>(static_cast<uintptr_t>(block));
  l.th = static_cast<double*>(PyArray_DATA(a));
  l.dF = static_cast<const double*>(PyArray_DATA(b));
  l.F = reinterpret_cast<const double*>(static_cast<uintptr_t>(F));
  l.G = reinterpret_cast<const double*>(static_cast<uintptr_t>(G));
  l.H = reinterpret_cast<const double*>(static_cast<uintptr_t>(H));
  l.seed = reinterpret_cast<uint64_t*>(static_cast<uintptr_t>(seed));
  l.n_theta = PyArray_DIM(a, 0);
  Py_RETURN_NONE;
}

int fe_traverse(PyObject* self_, visitproc visit, void* arg) {
  FastElbo* s = reinterpret_cast<FastElbo*>(self_);
#define X(f) Py_VISIT(s->f);
  FE_OBJECTS(X)
#undef X
  Py_VISIT(s->keep);
  return 0;
}

int fe_clear(PyObject* self_) {
  FastElbo* s = reinterpret_cast<FastElbo*>(self_);
  s->lane = StepLane();
#define X(f) Py_CLEAR(s->f);
  FE_OBJECTS(X)
#undef X
  Py_CLEAR(s->keep);
  return 0;
}

void fe_dealloc(PyObject* self_) {
  PyObject_GC_UnTrack(self_);
  fe_clear(self_);
  Py_TYPE(self_)->tp_free(self_);  // (a heap subclass's own dealloc releases the type)
}

PyMemberDef fe_members[] = {
#define X(f) {#f, T_OBJECT_EX, offsetof(FastElbo, f), 0, nullptr},
    FE_OBJECTS(X)
#undef X
    {nullptr, 0, 0, 0, nullptr}};

PyMethodDef fe_methods[] = {
    {"call", reinterpret_cast<PyCFunction>(reinterpret_cast<void (*)()>(fe_call)), METH_FASTCALL,
     "call(theta, seed): the repeat of the last fused _neg_elcbo call, or None when a re-check fails"},
    {"_bind_lane", fe_bind, METH_VARARGS, "addresses of the argument block the record repeats"},
    {nullptr, nullptr, 0, nullptr}};

PyTypeObject FastElboType = {PyVarObject_HEAD_INIT(nullptr, 0)};

PyObject* mod_setup(PyObject*, PyObject* args) {
  PyObject *globals, *lib_globals, *ctx_of_fn, *philox_fn;
  if (!PyArg_ParseTuple(args, "O!O!OO", &PyDict_Type, &globals, &PyDict_Type, &lib_globals, &ctx_of_fn, &philox_fn))
    return nullptr;
  Py_INCREF(globals);
  Py_INCREF(lib_globals);
  Py_XSETREF(g_lib_globals, lib_globals);
  Py_INCREF(ctx_of_fn);
  Py_INCREF(philox_fn);
  Py_XSETREF(g_globals, globals);
  Py_XSETREF(g_ctx_of, ctx_of_fn);
  Py_XSETREF(g_philox_seed, philox_fn);
  Py_RETURN_NONE;
}

PyMethodDef mod_methods[] = {
    {"setup", mod_setup, METH_VARARGS,
     "setup(module globals holding _FAST_PATH, _lib's globals holding _default_ctx, ctx_of, philox_seed)"},
    {nullptr, nullptr, 0, nullptr}};

PyModuleDef mod_def = {PyModuleDef_HEAD_INIT, "_step_native", "native repeat lane of _neg_elcbo", -1, mod_methods,
                       nullptr, nullptr, nullptr, nullptr};

}  // namespace

PyMODINIT_FUNC PyInit__step_native(void) {
  import_array();
  struct {
    PyObject** slot;
    const char* text;
  } names[] = {{&s_FAST_PATH, "_FAST_PATH"}, {&s_optimize_mu, "optimize_mu"}, {&s_optimize_sigma, "optimize_sigma"},
               {&s_optimize_lambd, "optimize_lambd"}, {&s_optimize_weights, "optimize_weights"}, {&s_D, "D"}, {&s_K, "K"},
               {&s_dict, "__dict__"}, {&s_fused_last, "_fused_last"}, {&s_ctx, "_ctx"}, {&s_lb, "lb"}, {&s_ub, "ub"},
               {&s_tol_con, "tol_con"}, {&s_weight_threshold, "weight_threshold"}, {&s_weight_penalty, "weight_penalty"},
               {&s_get, "get"}, {&s_posteriors, "posteriors"}, {&s_X, "X"}, {&s_shape, "shape"}, {&s_gp_quick, "_gp_quick"},
               {&s_alpha, "alpha"}, {&s_hyp, "hyp"}, {&s_side, "side"}, {&s_call_py, "_call_py"},
               {&s_finish_py, "_finish_py"}, {&s_default_ctx, "_default_ctx"}};
  for (auto& n : names)
    if (!(*n.slot = PyUnicode_InternFromString(n.text))) return nullptr;
  if (!(g_zero_f = PyFloat_FromDouble(0.0)) || !(g_zero_i = PyLong_FromLong(0))) return nullptr;
  FastElboType.tp_name = "pyvbmc_amd._step_native.FastElboBase";
  FastElboType.tp_basicsize = sizeof(FastElbo);
  FastElboType.tp_flags = Py_TPFLAGS_DEFAULT | Py_TPFLAGS_BASETYPE | Py_TPFLAGS_HAVE_GC;
  FastElboType.tp_doc = "what a repeat of the last fused _neg_elcbo call needs, and the repeat itself";
  FastElboType.tp_new = PyType_GenericNew;
  FastElboType.tp_dealloc = fe_dealloc;
  FastElboType.tp_traverse = fe_traverse;
  FastElboType.tp_clear = fe_clear;
  FastElboType.tp_members = fe_members;
  FastElboType.tp_methods = fe_methods;
  if (PyType_Ready(&FastElboType) < 0) return nullptr;
  PyObject* m = PyModule_Create(&mod_def);
  if (!m) return nullptr;
  // what variational_optimization.py expects of setup() and _bind_lane(); a build with another number is not used
  if (PyModule_AddIntConstant(m, "ABI", 1) < 0) {
    Py_DECREF(m);
    return nullptr;
  }
  Py_INCREF(&FastElboType);
  if (PyModule_AddObject(m, "FastElboBase", reinterpret_cast<PyObject*>(&FastElboType)) < 0) {
    Py_DECREF(&FastElboType);
    Py_DECREF(m);
    return nullptr;
  }
  return m;
}
