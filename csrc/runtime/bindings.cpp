// Python bindings of the host runtime (_native): ONNX reader, CPU executor, tree compiler,
// risk.v1 wire codec, account index, XXH64.
#include <pybind11/numpy.h>
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include <atomic>
#include <cstring>
#include <memory>
#include <thread>

#include "account_index.h"
#include "acct_core.h"
#include "acct_devices.h"
#include "audit.h"
#include "h2grpc.h"
#include "cpu_device.h"
#include "cpu_scorer.h"
#include "serve_core.h"
#include "link_index.h"
#include "mult_sketch.h"
#include "executor.h"
#include "onnx_model.h"
#include "sampler.h"
#include "trees.h"
#include "wire.h"
#include "xxh64.h"

namespace py = pybind11;
using namespace igp;

namespace {

py::object attr_value(const onnx::Attribute& a) {
  switch (a.type) {
    case onnx::A_FLOAT: return py::float_(a.f);
    case onnx::A_INT: return py::int_(a.i);
    case onnx::A_STRING: return py::str(a.s);
    case onnx::A_FLOATS: return py::array_t<float>(a.floats.size(), a.floats.data());
    case onnx::A_INTS: return py::array_t<int64_t>(a.ints.size(), a.ints.data());
    case onnx::A_STRINGS: {
      py::list l;
      for (auto& s : a.strings) l.append(py::str(s));
      return l;
    }
    case onnx::A_TENSOR: {
      if (!a.t) return py::none();
      std::vector<py::ssize_t> shape(a.t->dims.begin(), a.t->dims.end());
      if (a.t->dtype == onnx::FLOAT) return py::array_t<float>(shape, a.t->f.data());
      return py::array_t<int64_t>(shape, a.t->i.data());
    }
    default: return py::none();
  }
}

py::array tensor_to_np(const onnx::Tensor& t) {
  std::vector<py::ssize_t> shape(t.dims.begin(), t.dims.end());
  if (t.dtype == onnx::FLOAT) return py::array_t<float>(shape, t.f.data());
  return py::array_t<int64_t>(shape, t.i.data());
}

onnx::Tensor np_to_tensor(const std::string& name, py::array arr) {
  onnx::Tensor t;
  t.name = name;
  for (py::ssize_t d = 0; d < arr.ndim(); ++d) t.dims.push_back(arr.shape(d));
  if (py::isinstance<py::array_t<int64_t>>(arr) || arr.dtype().kind() == 'i') {
    auto a = py::array_t<int64_t, py::array::c_style | py::array::forcecast>(arr);
    // an int32 array keeps its element type (ONNX types GRU / LSTM sequence_lens tensor(int32))
    t.dtype = arr.dtype().kind() == 'i' && arr.itemsize() == 4 ? onnx::INT32 : onnx::INT64;
    t.i.assign(a.data(), a.data() + a.size());
  } else {
    auto a = py::array_t<float, py::array::c_style | py::array::forcecast>(arr);
    t.dtype = onnx::FLOAT;
    t.f.assign(a.data(), a.data() + a.size());
  }
  return t;
}

py::list value_infos(const std::vector<onnx::ValueInfo>& vs) {
  py::list l;
  for (auto& v : vs) l.append(py::make_tuple(v.name, v.elem_type, v.dims, v.params));
  return l;
}

template <class T>
py::array_t<T> vec_np(const std::vector<T>& v) { return py::array_t<T>(v.size(), v.data()); }

// Python handle of a serving core: keeps the device object (whose function table the core
// calls) alive for as long as the core may use it.
struct PyServe {
  std::shared_ptr<ServeCore> core;
  py::object dev;
};

// Python handle of the account-RPC router: keeps the model devices (whose function tables its
// cores call) alive for as long as the cores may use them
struct PyAcct {
  std::shared_ptr<AcctRouter> router;
  std::vector<py::object> devs;
  ~PyAcct() {
    if (router) {
      py::gil_scoped_release rel;
      router->stop();
    }
  }
};

const IgpModelOps* model_ops_of(py::object dev) {
  const uintptr_t p = dev.attr("model_ops")().cast<uintptr_t>();
  if (!p) throw std::runtime_error("model_ops(): null function table");
  return reinterpret_cast<const IgpModelOps*>(p);
}

py::dict acct_stats_dict(const AcctStats& t) {
  py::dict d;
  d["items"] = t.items; d["steps"] = t.steps; d["rows"] = t.rows; d["device_ns"] = t.device_ns;
  d["queue_ns"] = t.queue_ns; d["finish_ns"] = t.finish_ns; d["wait_errors"] = t.wait_errors;
  d["submit_ns"] = t.submit_ns; d["turn_ns"] = t.turn_ns; d["free_ns"] = t.free_ns;
  d["full_steps"] = t.full_steps; d["idle_steps"] = t.idle_steps; d["aged_steps"] = t.aged_steps;
  d["max_step_rows"] = t.max_step_rows;
  return d;
}

// the native gRPC server; stopped without the GIL (its cold threads may be waiting for it)
struct PyGrpc {
  std::unique_ptr<GrpcServer> srv;
  py::object core;  // keeps the PyServe (and its device) alive
  py::object acct;  // keeps the PyAcct alive
  ~PyGrpc() {
    if (srv) {
      {
        py::gil_scoped_release rel;
        srv->stop();
      }
      srv.reset();  // drops the Python callable: with the GIL
    }
  }
};

const IgpDeviceOps* device_ops_of(py::object dev) {
  const uintptr_t p = dev.attr("device_ops")().cast<uintptr_t>();
  if (!p) throw std::runtime_error("device_ops(): null function table");
  return reinterpret_cast<const IgpDeviceOps*>(p);
}

}  // namespace

PYBIND11_MODULE(_native, m) {
  m.doc() = "igaming_platform_amd host runtime (C++)";

  m.def("xxh64", [](py::bytes b, uint64_t seed) {
    std::string s = b;
    return xxh64(s.data(), s.size(), seed);
  });
  m.def("id_hashes", [](const std::vector<std::string>& ids, uint64_t seed) {
    py::array_t<uint64_t> out(ids.size());
    auto* o = out.mutable_data();
    for (size_t k = 0; k < ids.size(); ++k) o[k] = id_hash(ids[k], seed);
    return out;
  });

  py::class_<onnx::Model, std::shared_ptr<onnx::Model>>(m, "OnnxModel")
      .def_static("from_bytes", [](py::bytes b) { return std::make_shared<onnx::Model>(onnx::parse_model(std::string(b))); })
      .def_static("load", [](const std::string& p) { return std::make_shared<onnx::Model>(onnx::load_model(p)); })
      .def_readonly("ir_version", &onnx::Model::ir_version)
      .def_readonly("producer_name", &onnx::Model::producer_name)
      .def_readonly("opsets", &onnx::Model::opsets)
      .def_readonly("metadata", &onnx::Model::metadata)
      .def("inputs", [](const onnx::Model& mm) { return value_infos(mm.graph.inputs); })
      .def("outputs", [](const onnx::Model& mm) { return value_infos(mm.graph.outputs); })
      .def("initializer_names", [](const onnx::Model& mm) {
        std::vector<std::string> n;
        for (auto& kv : mm.graph.initializers) n.push_back(kv.first);
        return n;
      })
      .def("initializer", [](const onnx::Model& mm, const std::string& name) {
        auto it = mm.graph.initializers.find(name);
        if (it == mm.graph.initializers.end()) throw py::key_error(name);
        return tensor_to_np(it->second);
      })
      // ONNX element type of an initializer as the file stores it (uint8 / int8 / int32 arrive widened to int64)
      .def("initializer_dtype", [](const onnx::Model& mm, const std::string& name) {
        auto it = mm.graph.initializers.find(name);
        if (it == mm.graph.initializers.end()) throw py::key_error(name);
        return it->second.elem;
      })
      .def("nodes", [](const onnx::Model& mm) {
        py::list l;
        for (auto& n : mm.graph.nodes) {
          py::dict d, attrs;
          d["op_type"] = n.op_type;
          d["domain"] = n.domain;
          d["name"] = n.name;
          d["inputs"] = n.inputs;
          d["outputs"] = n.outputs;
          for (auto& kv : n.attrs) attrs[py::str(kv.first)] = attr_value(kv.second);
          d["attrs"] = attrs;
          l.append(d);
        }
        return l;
      });

  py::class_<exec::Executor, std::shared_ptr<exec::Executor>>(m, "Executor")
      .def(py::init([](std::shared_ptr<onnx::Model> mm) { return std::make_shared<exec::Executor>(*mm); }))
      .def("run", [](const exec::Executor& ex, py::dict inputs) {
        std::map<std::string, onnx::Tensor> in;
        for (auto item : inputs) {
          std::string name = py::str(item.first);
          in[name] = np_to_tensor(name, py::array::ensure(item.second));
        }
        std::map<std::string, onnx::Tensor> out;
        {
          py::gil_scoped_release rel;
          out = ex.run(in);
        }
        py::dict res;
        for (auto& kv : out) res[py::str(kv.first)] = tensor_to_np(kv.second);
        return res;
      })
      .def("tree_info", [](const exec::Executor& ex, size_t node_index) {
        const trees::Ensemble* e = ex.ensemble(node_index);
        if (!e) throw std::runtime_error("node is not a TreeEnsemble");
        size_t n_nodes = 0;
        for (auto& tr : e->trees) n_nodes += tr.size();
        py::dict d;
        d["depth"] = e->max_depth;
        d["n_trees"] = e->n_trees();
        d["n_nodes"] = n_nodes;
        d["k"] = e->n_targets;
        d["aggregate"] = e->aggregate;
        d["post"] = e->post;
        d["n_member"] = e->n_member;
        return d;
      }, py::arg("node_index"))
      .def("tree_sparse", [](const exec::Executor& ex, size_t node_index) {
        const trees::Ensemble* e = ex.ensemble(node_index);
        if (!e) throw std::runtime_error("node is not a TreeEnsemble");
        trees::Sparse sp = trees::to_sparse(*e);
        const int64_t N = int64_t(sp.nodes.size() / 4), L = int64_t(sp.leaf_w.size() / std::max(sp.k, 1));
        py::dict d;
        d["depth"] = sp.depth;
        d["n_trees"] = sp.n_trees;
        d["k"] = sp.k;
        d["nodes"] = py::array_t<int32_t>({N, int64_t(4)}, sp.nodes.data());
        d["roots"] = vec_np(sp.roots);
        d["leaf_w"] = py::array_t<float>({L, int64_t(sp.k)}, sp.leaf_w.data());
        d["leaf_has"] = py::array_t<uint8_t>({L, int64_t(sp.k)}, sp.leaf_has.data());
        d["sets"] = vec_np(sp.sets);
        d["base_values"] = vec_np(e->base_values);
        d["post"] = e->post;
        d["aggregate"] = e->aggregate;
        d["classifier"] = e->classifier;
        d["binary_case"] = e->binary_case;
        d["binary_class"] = e->binary_class & 1;
        d["weights_all_positive"] = !(e->binary_class & 0x100);
        d["n_outputs"] = e->n_outputs;
        d["max_feature"] = e->max_feature;
        d["classlabels"] = vec_np(e->classlabels);
        return d;
      }, py::arg("node_index"))
      .def("tree_complete", [](const exec::Executor& ex, size_t node_index, int32_t limit) {
        const trees::Ensemble* e = ex.ensemble(node_index);
        if (!e) throw std::runtime_error("node is not a TreeEnsemble");
        trees::Complete c = trees::to_complete(*e, limit);
        const int64_t n_int = (int64_t(1) << c.depth) - 1, n_leaf = int64_t(1) << c.depth;
        py::dict d;
        d["depth"] = c.depth;
        d["n_trees"] = c.n_trees;
        d["k"] = c.k;
        d["nodes"] = py::array_t<float>({int64_t(c.n_trees), n_int, int64_t(2)}, c.nodes.data());
        d["leaves"] = py::array_t<float>({int64_t(c.n_trees), n_leaf, int64_t(c.k)}, c.leaves.data());
        d["sets"] = vec_np(c.sets);
        d["base_values"] = vec_np(e->base_values);
        d["post"] = e->post;
        d["aggregate"] = e->aggregate;
        d["classifier"] = e->classifier;
        d["binary_case"] = e->binary_case;
        d["binary_class"] = e->binary_class & 1;
        d["weights_all_positive"] = !(e->binary_class & 0x100);
        d["n_outputs"] = e->n_outputs;
        d["max_feature"] = e->max_feature;
        d["classlabels"] = vec_np(e->classlabels);
        return d;
      }, py::arg("node_index"), py::arg("limit") = 12)
      // the compiled form of an SVMClassifier / SVMRegressor node (csrc/runtime/svm.h)
      .def("svm_info", [](const exec::Executor& ex, size_t node_index) {
        const svm::SvmModel* m = ex.svm_model(node_index);
        if (!m) throw std::runtime_error("node is not an SVMClassifier / SVMRegressor");
        py::dict d;
        d["classifier"] = m->classifier;
        d["kernel"] = m->kernel;
        d["gamma"] = m->gamma;
        d["coef0"] = m->coef0;
        d["degree"] = m->degree;
        d["n_sv"] = m->n_sv;
        d["n_feat"] = m->n_feat;
        d["sv"] = py::array_t<float>({m->n_sv, m->n_feat}, m->sv.data());
        d["coef"] = vec_np(m->coef);
        d["rho"] = m->rho;
        d["post"] = m->post;
        d["one_class"] = m->one_class;
        d["platt"] = m->platt;
        d["prob_a"] = m->prob_a;
        d["prob_b"] = m->prob_b;
        d["classlabels"] = vec_np(m->classlabels);
        return d;
      }, py::arg("node_index"));

  py::class_<wire::RequestBatch, std::shared_ptr<wire::RequestBatch>>(m, "RequestBatch")
      .def(py::init<>())
      .def("parse_batch", [](wire::RequestBatch& b, py::bytes data) {
        char* p; py::ssize_t n;
        PYBIND11_BYTES_AS_STRING_AND_SIZE(data.ptr(), &p, &n);
        py::gil_scoped_release rel;
        wire::parse_batch(p, size_t(n), b);
      })
      .def("parse_tx", [](wire::RequestBatch& b, py::bytes data) {
        char* p; py::ssize_t n;
        PYBIND11_BYTES_AS_STRING_AND_SIZE(data.ptr(), &p, &n);
        const std::string& own = b.own(p, size_t(n));
        wire::parse_tx(own.data(), own.size(), b);
      })
      .def("parse_tx_list", [](wire::RequestBatch& b, py::list items) {
        // micro-batcher path: many unary ScoreTransactionRequest payloads -> one columnar batch
        std::vector<std::pair<const char*, size_t>> bufs;
        bufs.reserve(items.size());
        for (auto it : items) {
          char* p; py::ssize_t n;
          if (PYBIND11_BYTES_AS_STRING_AND_SIZE(it.ptr(), &p, &n) != 0) throw std::runtime_error("parse_tx_list: bytes expected");
          bufs.emplace_back(p, size_t(n));
        }
        py::gil_scoped_release rel;
        b.reserve(b.size() + bufs.size());
        size_t total = 0;
        for (auto& x : bufs) total += x.second;
        std::string all;  // one arena copy for the whole micro-batch
        all.reserve(total);
        for (auto& x : bufs) all.append(x.first, x.second);
        const std::string& own = b.own(all.data(), all.size());
        size_t off = 0;
        for (auto& x : bufs) {
          wire::parse_tx(own.data() + off, x.second, b);
          off += x.second;
        }
      })
      .def("pack_reqrec", [](const wire::RequestBatch& b, py::array_t<int32_t, py::array::c_style> slots,
                             py::array out, int64_t ts, py::object owners) {
        // fill REQREC rows (48 B: slot, tx_type | owner<<8, amount, dev, fp, ip, ts) in place
        const size_t n = b.size();
        if (size_t(slots.size()) != n) throw std::runtime_error("pack_reqrec: slots length");
        if (size_t(out.nbytes()) < n * sizeof(ReqRec)) throw std::runtime_error("pack_reqrec: output too small");
        if (!(out.flags() & py::array::c_style)) throw std::runtime_error("pack_reqrec: output must be contiguous");
        const int32_t* own = nullptr;
        py::array_t<int32_t, py::array::c_style | py::array::forcecast> own_arr;
        if (!owners.is_none()) {
          own_arr = owners;
          if (size_t(own_arr.size()) != n) throw std::runtime_error("pack_reqrec: owners length");
          own = own_arr.data();
        }
        ReqRec* o = reinterpret_cast<ReqRec*>(out.mutable_data());
        const int32_t* sl = slots.data();
        py::gil_scoped_release rel;
        for (size_t k = 0; k < n; ++k) {
          o[k].slot = sl[k];
          o[k].tx_type = int32_t(b.tx_type[k]) | (own ? (own[k] << 8) : 0);
          o[k].amount = b.amount[k];
          o[k].dev_hash = b.device_hash[k];
          o[k].fp_hash = b.fp_hash[k];
          o[k].ip_hash = b.ip_hash[k];
          o[k].ts = ts;
        }
      }, py::arg("slots"), py::arg("out"), py::arg("ts"), py::arg("owners") = py::none())
      .def("clear", &wire::RequestBatch::clear)
      .def("__len__", &wire::RequestBatch::size)
      .def_property_readonly("account_id", [](const wire::RequestBatch& b) {
        py::list l(b.account_id.size());
        for (size_t k = 0; k < b.account_id.size(); ++k)
          l[k] = py::str(b.account_id[k].data(), b.account_id[k].size());
        return l;
      })
      .def("columns", [](const wire::RequestBatch& b) {
        py::dict d;
        d["account_hash"] = vec_np(b.account_hash);
        d["amount"] = vec_np(b.amount);
        d["tx_type"] = vec_np(b.tx_type);
        d["device_hash"] = vec_np(b.device_hash);
        d["fp_hash"] = vec_np(b.fp_hash);
        d["ip_hash"] = vec_np(b.ip_hash);
        return d;
      });

  // the serving core's bound on one account's rows in a step (mult_sketch.h): `slots` holds the
  // rows of the step's items back to back, `sizes` the rows per item. Each item is sketched as
  // on the ingress threads, the items are combined as in the stepper.
  m.attr("K1_SEG_MAX") = IGP_K1_SEG_MAX;
  m.def("mult_step_bound", [](py::array_t<int32_t, py::array::c_style | py::array::forcecast> slots,
                              std::vector<int64_t> sizes) {
    const int32_t* sp = slots.data();
    const int64_t total = slots.size();
    std::vector<MultSketch> items(sizes.size());
    std::vector<ReqRec> rows;
    int64_t at = 0;
    for (size_t i = 0; i < sizes.size(); ++i) {
      if (sizes[i] < 0 || at + sizes[i] > total) throw std::runtime_error("mult_step_bound: sizes exceed slots");
      rows.assign(size_t(sizes[i]), ReqRec{});
      for (int64_t k = 0; k < sizes[i]; ++k) rows[size_t(k)].slot = sp[at + k];
      items[i].build(rows.data(), rows.size());
      at += sizes[i];
    }
    if (at != total) throw std::runtime_error("mult_step_bound: sizes do not cover slots");
    std::vector<const MultSketch*> parts;
    for (const MultSketch& it : items) parts.push_back(&it);
    std::vector<uint32_t> scratch;
    return mult_step_bound(parts.data(), parts.size(), scratch);
  }, py::arg("slots"), py::arg("sizes"));

  m.def("tx_type_id", [](const std::string& s) { return int(wire::tx_type_id(s.data(), s.size())); });
  // batch identifier digests (utils/hashing.id_hash semantics: "" -> 0, a real 0 -> 1)
  m.def("id_hashes", [](py::list values, uint64_t seed) {
    std::vector<std::string_view> v;
    v.reserve(values.size());
    for (auto it : values) {
      char* p; py::ssize_t n;
      if (PyUnicode_Check(it.ptr())) {
        const char* u = PyUnicode_AsUTF8AndSize(it.ptr(), &n);
        if (!u) throw py::error_already_set();
        p = const_cast<char*>(u);
      } else if (PYBIND11_BYTES_AS_STRING_AND_SIZE(it.ptr(), &p, &n) != 0) {
        throw std::runtime_error("id_hashes: str or bytes expected");
      }
      v.emplace_back(p, size_t(n));
    }
    py::array_t<uint64_t> out(v.size());
    uint64_t* o = out.mutable_data();
    {
      py::gil_scoped_release rel;
      for (size_t k = 0; k < v.size(); ++k) o[k] = id_hash(v[k], seed);
    }
    return out;
  });

  // the inline key of an id (form bits, 16 bytes); scalar: the table decode the SSSE3 path replaced
  m.def("account_key", [](const std::string& id, bool scalar) {
    uint8_t key[16];
    const uint32_t form = AccountIndex::encode_key(id, key, scalar);
    return py::make_tuple(form, py::bytes(reinterpret_cast<const char*>(key), 16));
  }, py::arg("id"), py::arg("scalar") = false);
  py::class_<AccountIndex, std::shared_ptr<AccountIndex>>(m, "AccountIndex")
      .def(py::init<int64_t>())
      // node-shared index (/dev/shm/<shm_name>): one creator sizes it, the other ranks open it
      .def(py::init<int64_t, const std::string&, bool>(), py::arg("capacity"), py::arg("shm_name"), py::arg("create"))
      .def("lookup_batch", [](AccountIndex& ix, const wire::RequestBatch& b, bool insert, py::object sel) {
        // sel: optional bool/uint8 mask (rows of other owners are skipped, slot -1)
        py::array_t<int32_t> slots(b.size());
        py::array_t<uint8_t> fresh(b.size());
        py::array_t<uint8_t, py::array::c_style | py::array::forcecast> m;
        const uint8_t* mp = nullptr;
        if (!sel.is_none()) {
          m = sel;
          if (size_t(m.size()) != b.size()) throw std::runtime_error("lookup_batch: mask length");
          mp = m.data();
        }
        int32_t* sp = slots.mutable_data();
        uint8_t* fp = fresh.mutable_data();
        {
          py::gil_scoped_release rel;
          ix.lookup_views(b.account_id.data(), b.account_hash.data(), b.size(), insert, sp, fp, mp);
        }
        return py::make_tuple(slots, fresh);
      }, py::arg("batch"), py::arg("insert") = true, py::arg("sel") = py::none())
      .def("lookup", [](AccountIndex& ix, const std::vector<std::string>& ids, bool insert, py::object hashes) {
        std::vector<uint64_t> h(ids.size());
        if (hashes.is_none()) {
          for (size_t k = 0; k < ids.size(); ++k) h[k] = id_hash(ids[k], SEED_ACCOUNT);
        } else {  // explicit digests (tests: forced collisions)
          h = hashes.cast<std::vector<uint64_t>>();
          if (h.size() != ids.size()) throw std::runtime_error("lookup: hashes length");
        }
        py::array_t<int32_t> slots(ids.size());
        py::array_t<uint8_t> fresh(ids.size());
        ix.lookup(ids, h, insert, slots.mutable_data(), fresh.mutable_data());
        return py::make_tuple(slots, fresh);
      }, py::arg("ids"), py::arg("insert") = false, py::arg("hashes") = py::none())
      .def("__len__", &AccountIndex::size)
      .def_property_readonly("capacity", &AccountIndex::capacity)
      .def_property_readonly("collisions", &AccountIndex::collisions)
      .def_property_readonly("shared", &AccountIndex::shared)
      .def("unlink_shared", &AccountIndex::unlink_shared)
      .def("id_of", &AccountIndex::id_of);

  py::class_<LinkIndex, std::shared_ptr<LinkIndex>>(m, "LinkIndex")
      .def(py::init<int, int64_t>(), py::arg("per_key") = 8, py::arg("buckets") = int64_t(1) << 18)
      .def(py::init<int, int64_t, const std::string&, bool>(), py::arg("per_key"), py::arg("buckets"),
           py::arg("shm_name"), py::arg("create"))
      .def("unlink_shared", &LinkIndex::unlink_shared)
      .def_property_readonly("shared", &LinkIndex::shared)
      .def("add", [](LinkIndex& ix, py::array_t<uint64_t, py::array::c_style | py::array::forcecast> dev,
                     py::array_t<int64_t, py::array::c_style | py::array::forcecast> acct) {
        if (dev.size() != acct.size()) throw std::runtime_error("LinkIndex.add: length mismatch");
        const uint64_t* d = dev.data();
        const int64_t* a = acct.data();
        const size_t n = size_t(dev.size());
        py::gil_scoped_release rel;
        ix.add(d, a, n);
      })
      .def("linked", &LinkIndex::linked, py::arg("acct"), py::arg("limit") = 16)
      .def("devices_of", &LinkIndex::devices_of)
      .def("n_devices", &LinkIndex::n_devices)
      .def("_debug_acquire_and_leak", &LinkIndex::debug_acquire_and_leak)
      .def_property_readonly("takeovers", &LinkIndex::takeovers)
      .def_property_readonly("read_timeouts", &LinkIndex::read_timeouts);

  py::class_<CpuScorer, std::shared_ptr<CpuScorer>>(m, "CpuScorer")
      .def(py::init<int64_t, int, int, int, int>(), py::arg("capacity"), py::arg("ring_size") = 256,
           py::arg("event_ring") = 100, py::arg("event_dim") = 16, py::arg("ext_width") = 0)
      .def("set_cfg", [](CpuScorer& c, py::array_t<uint8_t, py::array::c_style | py::array::forcecast> b) {
        if (b.size() != (py::ssize_t)sizeof(ScoreCfg)) throw std::runtime_error("ScoreCfg must be 176 bytes");
        ScoreCfg cfg;
        std::memcpy(&cfg, b.data(), sizeof cfg);
        c.set_cfg(cfg);
      })
      .def("set_tables", [](CpuScorer& c, py::array_t<uint64_t, py::array::c_style | py::array::forcecast> bk,
                            py::array_t<uint32_t, py::array::c_style | py::array::forcecast> be,
                            py::array_t<uint64_t, py::array::c_style | py::array::forcecast> ik,
                            py::array_t<uint32_t, py::array::c_style | py::array::forcecast> iv) {
        if (bk.size() != be.size() || ik.size() != iv.size()) throw std::runtime_error("table sizes");
        c.set_tables(bk.data(), be.data(), bk.size(), ik.data(), iv.data(), ik.size());
      })
      .def("set_model", [](CpuScorer& c, py::object ex, std::string in, std::string out, int col) {
        if (ex.is_none()) { c.set_model(nullptr, "", "", 0); return; }
        c.set_model(ex.cast<std::shared_ptr<exec::Executor>>(), in, out, col);
      })
      .def("set_batch", [](CpuScorer& c, py::array_t<int32_t, py::array::c_style | py::array::forcecast> slots,
                           py::array rows) {
        if ((size_t)rows.nbytes() != (size_t)slots.size() * sizeof(AcctBatch)) throw std::runtime_error("rows");
        c.set_batch(slots.data(), reinterpret_cast<const AcctBatch*>(rows.data()), slots.size());
      })
      .def("set_ext", [](CpuScorer& c, py::array_t<int32_t, py::array::c_style | py::array::forcecast> slots,
                         py::array_t<float, py::array::c_style | py::array::forcecast> e) {
        if (e.ndim() != 2 || e.shape(0) != slots.size()) throw std::runtime_error("ext must be [n, w]");
        c.set_ext(slots.data(), e.data(), slots.size(), (int)e.shape(1));
      })
      .def("reset", [](CpuScorer& c, py::array_t<int32_t, py::array::c_style | py::array::forcecast> slots) {
        c.reset(slots.data(), slots.size());
      })
      .def("ingest", [](CpuScorer& c, py::array req) {
        if (req.nbytes() % sizeof(ReqRec)) throw std::runtime_error("ReqRec rows expected");
        const ReqRec* r = reinterpret_cast<const ReqRec*>(req.data());
        const size_t n = req.nbytes() / sizeof(ReqRec);
        py::gil_scoped_release rel;
        c.ingest(r, n);
      })
      .def("score", [](CpuScorer& c, py::array req, int64_t now, bool update, bool want_features) {
        if (req.nbytes() % sizeof(ReqRec)) throw std::runtime_error("ReqRec rows expected");
        const size_t n = req.nbytes() / sizeof(ReqRec);
        py::array_t<uint32_t> res({(py::ssize_t)n, (py::ssize_t)2});
        py::object feat = py::none();
        FeatRec* fp = nullptr;
        if (want_features) {
          py::array_t<int32_t> f({(py::ssize_t)n, (py::ssize_t)32});
          fp = reinterpret_cast<FeatRec*>(f.mutable_data());
          feat = f;
        }
        const ReqRec* r = reinterpret_cast<const ReqRec*>(req.data());
        ResultRec* rp = reinterpret_cast<ResultRec*>(res.mutable_data());
        {
          py::gil_scoped_release rel;
          c.score(r, n, now, update, rp, fp);
        }
        return py::make_tuple(res, feat);
      }, py::arg("req"), py::arg("now"), py::arg("update") = true, py::arg("want_features") = true)
      .def("features", [](CpuScorer& c, int32_t slot, int64_t now) {
        FeatRec f = c.features(slot, now);
        py::array_t<int32_t> out(32);
        std::memcpy(out.mutable_data(), &f, sizeof f);
        return out;
      })
      .def("event_count", [](CpuScorer& c, int32_t slot) { return c.event_count(slot); })
      .def("event_history", [](CpuScorer& c, int32_t slot) {
        py::array_t<float> out({(py::ssize_t)c.event_ring(), (py::ssize_t)c.event_dim()});
        c.event_history(slot, out.mutable_data());
        return out;
      })
      .def("state", [](CpuScorer& c) {
        py::dict d;
        d["ring_ts"] = vec_np(c.ring_ts);
        d["ring_amt"] = vec_np(c.ring_amt);
        d["hll"] = vec_np(c.hll);
        d["rt"] = py::array_t<uint8_t>(c.rt.size() * sizeof(AcctRT), reinterpret_cast<const uint8_t*>(c.rt.data()));
        d["batch"] = py::array_t<uint8_t>(c.batch.size() * sizeof(AcctBatch),
                                          reinterpret_cast<const uint8_t*>(c.batch.data()));
        d["ext"] = vec_np(c.ext);
        d["ev"] = vec_np(c.ev);
        return d;
      })
      .def("load_state", [](CpuScorer& c, py::dict d) {
        auto load = [&](const char* k, void* dst, size_t nbytes) {
          py::array a = d[k].cast<py::array>();
          if ((size_t)a.nbytes() != nbytes) throw std::runtime_error(std::string("state size mismatch: ") + k);
          if (nbytes) std::memcpy(dst, py::array::ensure(a, py::array::c_style).data(), nbytes);  // empty: dst may be null
        };
        load("ring_ts", c.ring_ts.data(), c.ring_ts.size() * 4);
        load("ring_amt", c.ring_amt.data(), c.ring_amt.size() * 8);
        load("hll", c.hll.data(), c.hll.size());
        load("rt", c.rt.data(), c.rt.size() * sizeof(AcctRT));
        load("batch", c.batch.data(), c.batch.size() * sizeof(AcctBatch));
        load("ext", c.ext.data(), c.ext.size() * 4);
        load("ev", c.ev.data(), c.ev.size() * 2);
      })
      .def_property_readonly("capacity", &CpuScorer::capacity);

  // results: uint32[n,2] (ResultRec), feats: int32[n,32] (FeatRec) or None, ms: int64[n] or None
  auto view = [](py::array res, py::object feat, py::object ms, wire::ResultView& v,
                 py::array& keep_r, py::object& keep_f, py::object& keep_m) {
    keep_r = py::array_t<uint32_t, py::array::c_style | py::array::forcecast>(res);
    if (keep_r.ndim() != 2 || keep_r.shape(1) != 2) throw std::runtime_error("results must be [n,2] (ResultRec)");
    v.n = size_t(keep_r.shape(0));
    v.res = reinterpret_cast<const ResultRec*>(keep_r.data());
    v.feat = nullptr;
    v.response_ms = nullptr;
    if (!feat.is_none()) {
      auto f = py::array_t<int32_t, py::array::c_style | py::array::forcecast>(feat);
      if (f.ndim() != 2 || f.shape(1) != 32 || size_t(f.shape(0)) != v.n) throw std::runtime_error("features must be [n,32] (FeatRec)");
      keep_f = f;
      v.feat = reinterpret_cast<const FeatRec*>(f.data());
    }
    if (!ms.is_none()) {
      auto t = py::array_t<int64_t, py::array::c_style | py::array::forcecast>(ms);
      if (size_t(t.size()) != v.n) throw std::runtime_error("response_ms length mismatch");
      keep_m = t;
      v.response_ms = t.data();
    }
  };
  m.def("serialize_batch_response", [view](py::array res, py::object feat, py::object ms) {
    wire::ResultView v;
    py::array kr; py::object kf, km;
    view(res, feat, ms, v, kr, kf, km);
    std::string out;
    {
      py::gil_scoped_release rel;
      out = wire::serialize_batch_response(v);
    }
    return py::bytes(out);
  }, py::arg("results"), py::arg("features") = py::none(), py::arg("response_ms") = py::none());
  m.def("serialize_tx_response", [view](py::array res, py::object feat, py::object ms, size_t i) {
    wire::ResultView v;
    py::array kr; py::object kf, km;
    view(res, feat, ms, v, kr, kf, km);
    if (i >= v.n) throw std::runtime_error("index out of range");
    return py::bytes(wire::serialize_tx_response(v, i));
  }, py::arg("results"), py::arg("features") = py::none(), py::arg("response_ms") = py::none(), py::arg("index") = 0);
  m.def("serialize_tx_responses", [view](py::array res, py::object feat, py::object ms) {
    wire::ResultView v;
    py::array kr; py::object kf, km;
    view(res, feat, ms, v, kr, kf, km);
    std::vector<std::string> outs(v.n);
    {
      py::gil_scoped_release rel;
      for (size_t i = 0; i < v.n; ++i) outs[i] = wire::serialize_tx_response(v, i);
    }
    py::list l;
    for (auto& o : outs) l.append(py::bytes(o));
    return l;
  }, py::arg("results"), py::arg("features") = py::none(), py::arg("response_ms") = py::none());
  m.def("serialize_feature_vector", [](py::array feat) {
    auto f = py::array_t<int32_t, py::array::c_style | py::array::forcecast>(feat);
    if (f.size() != 32) throw std::runtime_error("FeatRec must have 32 int32 words");
    return py::bytes(wire::serialize_feature_vector(*reinterpret_cast<const FeatRec*>(f.data())));
  });

  // ---------------------------------------------------------------- native serving core
  py::class_<StepClock, std::shared_ptr<StepClock>>(m, "StepClock")
      .def(py::init<const std::string&, int, int, bool>(), py::arg("shm_name"), py::arg("world"), py::arg("rank"),
           py::arg("create"))
      .def(py::init<int>(), py::arg("world"))
      .def("issued", &StepClock::issued)
      .def("max_issued", &StepClock::max_issued)
      .def("hold_of", &StepClock::hold_of)
      .def("set_rank", &StepClock::set_rank)
      .def("unlink_shared", &StepClock::unlink_shared)
      .def_property_readonly("world", &StepClock::world)
      .def_property_readonly("rank", &StepClock::rank);

  py::class_<CpuDevice, std::shared_ptr<CpuDevice>>(m, "CpuDevice")
      .def(py::init<std::shared_ptr<CpuScorer>, int, int, bool>(), py::arg("scorer"), py::arg("depth") = 2,
           py::arg("cap") = 8192, py::arg("inplace") = true, py::keep_alive<1, 2>())
      .def("device_ops", [](const CpuDevice& d) { return reinterpret_cast<uintptr_t>(d.ops()); })
      .def("debug_fail_steps", &CpuDevice::debug_fail_steps, py::arg("n"), py::arg("after") = 0)
      .def("debug_hold_steps", &CpuDevice::debug_hold_steps, py::arg("n"))
      .def("debug_release_steps", &CpuDevice::debug_release_steps, py::call_guard<py::gil_scoped_release>())
      .def("debug_held_steps", &CpuDevice::debug_held_steps)
      .def_property_readonly("gathered_steps", &CpuDevice::gathered_steps);

  py::class_<ShmXchgDevice, std::shared_ptr<ShmXchgDevice>>(m, "ShmXchgDevice")
      .def(py::init<std::shared_ptr<CpuScorer>, const std::string&, int, int, int, int, bool, double>(),
           py::arg("scorer"), py::arg("shm_name"), py::arg("world"), py::arg("rank"), py::arg("depth"), py::arg("C"),
           py::arg("create"), py::arg("timeout_s") = 60.0, py::keep_alive<1, 2>())
      .def("device_ops", [](const ShmXchgDevice& d) { return reinterpret_cast<uintptr_t>(d.ops()); })
      .def_property_readonly("rows_scored", &ShmXchgDevice::rows_scored)
      .def_property_readonly("slot_violations", &ShmXchgDevice::slot_violations)
      .def_property_readonly("steps", &ShmXchgDevice::steps)
      .def("debug_stall_results_when", &ShmXchgDevice::debug_stall_results_when)
      .def("unlink_shared", &ShmXchgDevice::unlink_shared);

  py::class_<AuditRing, std::shared_ptr<AuditRing>>(m, "AuditRing")
      .def(py::init<int64_t>(), py::arg("capacity"))
      .def("pending", &AuditRing::pending)
      .def("append", [](AuditRing& a, py::array_t<uint32_t, py::array::c_style> res,
                        py::array_t<int32_t, py::array::c_style> slots, int owner, int64_t t_ms, int version) {
        const size_t n = size_t(slots.size());
        if (res.ndim() != 2 || size_t(res.shape(0)) != n || res.shape(1) != 2)
          throw std::runtime_error("AuditRing.append: res must be uint32[n,2] for n slots");
        const ResultRec* r = reinterpret_cast<const ResultRec*>(res.data());
        const int32_t* s = slots.data();
        py::gil_scoped_release rel;
        a.append(r, s, 1, owner, n, t_ms, uint16_t(version));
      }, py::arg("res"), py::arg("slots"), py::arg("owner"), py::arg("t_ms"), py::arg("version"))
      .def_property_readonly("evicted", &AuditRing::evicted)
      .def_property_readonly("appended", &AuditRing::appended)
      .def("flush_sqlite", [](AuditRing& a, const std::string& path, const std::string& schema,
                              std::vector<std::shared_ptr<AccountIndex>> idx) {
        py::gil_scoped_release rel;
        return a.flush_sqlite(path, schema, idx);
      })
      .def_property_readonly("capacity", &AuditRing::capacity)
      .def("flush_segment", [](AuditRing& a, const std::string& dir, const std::string& tag,
                               std::vector<std::shared_ptr<AccountIndex>> idx) {
        py::gil_scoped_release rel;
        return a.flush_segment(dir, tag, idx);
      })
      .def("peek", [](const AuditRing& a, int64_t max) {
        auto v = a.peek(max);
        py::dict d;
        std::vector<int64_t> t(v.size());
        std::vector<int32_t> sl(v.size()), ow(v.size()), ver(v.size());
        std::vector<uint32_t> pk(v.size());
        std::vector<float> ml(v.size());
        for (size_t i = 0; i < v.size(); ++i) {
          t[i] = v[i].t_ms; sl[i] = v[i].slot; ow[i] = v[i].owner; ver[i] = v[i].model_version;
          pk[i] = v[i].packed; ml[i] = v[i].ml;
        }
        d["t_ms"] = vec_np(t); d["slot"] = vec_np(sl); d["owner"] = vec_np(ow); d["model_version"] = vec_np(ver);
        d["packed"] = vec_np(pk); d["ml"] = vec_np(ml);
        return d;
      }, py::arg("max") = 1 << 20);

  m.def("audit_load_segment", [](const std::string& seg, const std::string& db, const std::string& schema) {
    py::gil_scoped_release rel;
    return audit_load_segment(seg, db, schema);
  }, py::arg("segment"), py::arg("db"), py::arg("schema"));

  py::class_<PyGrpc>(m, "GrpcServer")
      .def(py::init([](py::object core, py::function cold, int cold_threads, int batch_threads, py::object acct) {
             auto p = std::make_unique<PyGrpc>();
             std::shared_ptr<ServeCore> c;
             if (!core.is_none()) {
               c = core.cast<PyServe&>().core;
               p->core = core;
             }
             std::shared_ptr<AcctRouter> ar;
             if (!acct.is_none()) {
               ar = acct.cast<PyAcct&>().router;
               p->acct = acct;
             }
             // cold RPC: cold(path: str, body: bytes) -> bytes, or (grpc status, message)
             GrpcServer::ColdFn fn = [cb = py::function(cold)](const std::string& path, std::string body) {
               py::gil_scoped_acquire g;
               GrpcReply r;
               try {
                 py::object out = cb(py::str(path), py::bytes(body));
                 if (py::isinstance<py::bytes>(out)) {
                   r.body = out.cast<std::string>();
                 } else {
                   auto t = out.cast<py::tuple>();
                   r.status = t[0].cast<int>();
                   r.message = t[1].cast<std::string>();
                 }
               } catch (py::error_already_set& e) {
                 r.status = 13;
                 r.message = e.what();
               } catch (const std::exception& e) {
                 r.status = 13;
                 r.message = e.what();
               }
               return r;
             };
             p->srv = std::make_unique<GrpcServer>(c, std::move(fn), cold_threads, batch_threads, ar);
             return p;
           }),
           py::arg("core"), py::arg("cold"), py::arg("cold_threads") = 4, py::arg("batch_threads") = 8,
           py::arg("acct") = py::none())
      .def("start", [](PyGrpc& s, const std::string& host, int port, int workers) {
        py::gil_scoped_release rel;
        return s.srv->start(host, port, workers);
      }, py::arg("host"), py::arg("port"), py::arg("workers") = 4)
      .def("stop", [](PyGrpc& s) {
        py::gil_scoped_release rel;
        s.srv->stop();
      })
      .def("set_hot", [](PyGrpc& s, bool on) { s.srv->set_hot(on); })
      .def("stats", [](PyGrpc& s) {
        const auto st = s.srv->stats();
        py::dict d;
        d["calls"] = st.calls;
        d["hot_tx"] = st.hot_tx;
        d["hot_batch"] = st.hot_batch;
        d["cold"] = st.cold;
        d["errors"] = st.errors;
        d["connections"] = st.connections;
        d["hot_acct"] = st.hot_acct;
        d["hot_failures"] = st.hot_failures;
        return d;
      })
      .def("last_failure", [](PyGrpc& s) { return s.srv->last_failure(); });

  // host CPU sampler (csrc/runtime/sampler.h): tools/host_profile.py --sample
  m.def("sampler_start", [](int hz, size_t capacity) { sampler::start(hz, capacity); }, py::arg("hz") = 4000,
        py::arg("capacity") = size_t(1) << 20);
  m.def("sampler_stop", []() {
    const auto v = sampler::stop();
    py::array_t<uint64_t> pc(v.size());
    py::array_t<int32_t> tid(v.size());
    auto p = pc.mutable_unchecked<1>();
    auto t = tid.mutable_unchecked<1>();
    for (size_t i = 0; i < v.size(); ++i) {
      p(i) = v[i].pc;
      t(i) = v[i].tid;
    }
    return py::make_tuple(pc, tid);
  });
  m.def("grpc_load", [](const std::string& host, int port, const std::string& path, std::vector<std::string> payloads,
                        double rate, double seconds, int conns, int max_inflight) {
    LoadResult r;
    {
      py::gil_scoped_release rel;
      r = grpc_load(host, port, path, payloads, rate, seconds, conns, max_inflight);
    }
    py::dict d;
    d["latency_ms"] = vec_np(r.latency_ms);
    d["sched_ms"] = vec_np(r.sched_ms);
    d["errors"] = r.errors;
    d["sent"] = r.sent;
    d["seconds"] = r.seconds;
    d["elapsed"] = r.elapsed;
    return d;
  }, py::arg("host"), py::arg("port"), py::arg("path"), py::arg("payloads"), py::arg("rate"), py::arg("seconds"),
     py::arg("conns") = 8, py::arg("max_inflight") = 4096);

  py::class_<PyServe, std::shared_ptr<PyServe>>(m, "ServeCore")
      .def(py::init([](std::vector<std::shared_ptr<AccountIndex>> idx, py::object dev, int rank,
                       std::shared_ptr<StepClock> clock, int max_wait_us, int64_t timeout_us, int finishers,
                       bool features, int32_t seq0, int unary_depth) {
             ServeCore::Options o;
             o.unary_depth = unary_depth;
             o.max_wait_us = max_wait_us;
             o.timeout_us = timeout_us;
             o.finishers = finishers;
             o.features = features;
             o.seq0 = seq0;
             const IgpDeviceOps* ops = device_ops_of(dev);
             auto p = std::make_shared<PyServe>();
             p->dev = dev;
             py::gil_scoped_release rel;
             p->core = std::make_shared<ServeCore>(std::move(idx), ops, rank, std::move(clock), o);
             return p;
           }),
           py::arg("indexes"), py::arg("device"), py::arg("rank") = 0, py::arg("clock") = nullptr,
           py::arg("max_wait_us") = 200, py::arg("timeout_us") = -1, py::arg("finishers") = 2,
           py::arg("features") = true, py::arg("seq0") = 0, py::arg("unary_depth") = 0)
      .def("score_batch", [](PyServe& s, py::bytes data, int64_t now, int64_t t0_ns) {
        char* p; py::ssize_t n;
        PYBIND11_BYTES_AS_STRING_AND_SIZE(data.ptr(), &p, &n);
        std::string_view out;
        {
          py::gil_scoped_release rel;
          out = s.core->score_batch_view(p, size_t(n), now, t0_ns);
        }
        // The response is serialised into the thread's resident scratch buffer and copied once
        // into a bytes object of exactly its size (allocated under the GIL, filled without: the
        // MB-sized copy would otherwise serialise every ingress thread on the GIL). Letting the
        // core write into the bytes object itself (ServeCore::score_batch_into), allocated at
        // the response's upper bound or at a typical size and shrunk with _PyBytes_Resize, was
        // measured and is slower: glibc sets its mmap threshold from the SHRUNK size of the
        // block it frees, so the next, larger allocation is mmap'd afresh and pays a page fault
        // per 4 KB written on every call (299 per 1.2 MB response against 0 for an exact-size
        // allocation; profiles/NOTES.md round 9)
        PyObject* b = PyBytes_FromStringAndSize(nullptr, py::ssize_t(out.size()));
        if (!b) throw py::error_already_set();
        {
          py::gil_scoped_release rel;
          if (!out.empty()) std::memcpy(PyBytes_AS_STRING(b), out.data(), out.size());
        }
        return py::reinterpret_steal<py::bytes>(b);
      }, py::arg("data"), py::arg("now") = -1, py::arg("t0_ns") = 0)
      .def("score_rows", [](PyServe& s, py::array req, py::object owners, int64_t now, bool want_features) {
        if (req.nbytes() % sizeof(ReqRec)) throw std::runtime_error("score_rows: ReqRec rows expected");
        auto rq = py::array::ensure(req, py::array::c_style);
        const size_t n = size_t(rq.nbytes()) / sizeof(ReqRec);
        py::array_t<int32_t, py::array::c_style | py::array::forcecast> own;
        const int32_t* op = nullptr;
        if (!owners.is_none()) {
          own = owners;
          if (size_t(own.size()) != n) throw std::runtime_error("score_rows: owners length");
          op = own.data();
        }
        py::array_t<uint32_t> res({(py::ssize_t)n, (py::ssize_t)2});
        py::object feat = py::none();
        FeatRec* fp = nullptr;
        if (want_features) {
          py::array_t<int32_t> f({(py::ssize_t)n, (py::ssize_t)32});
          fp = reinterpret_cast<FeatRec*>(f.mutable_data());
          feat = f;
        }
        const ReqRec* r = reinterpret_cast<const ReqRec*>(rq.data());
        ResultRec* rp = reinterpret_cast<ResultRec*>(res.mutable_data());
        {
          py::gil_scoped_release rel;
          s.core->score_rows(r, op, n, now, want_features, rp, fp);
        }
        return py::make_tuple(res, feat);
      }, py::arg("req"), py::arg("owners") = py::none(), py::arg("now") = -1, py::arg("want_features") = true)
      .def("submit_tx", [](PyServe& s, py::bytes data, uint64_t tag, int64_t now, int64_t t0_ns) {
        char* p; py::ssize_t n;
        PYBIND11_BYTES_AS_STRING_AND_SIZE(data.ptr(), &p, &n);
        s.core->submit_tx(p, size_t(n), tag, now, t0_ns);  // parse + resolve of one row: GIL kept
      }, py::arg("data"), py::arg("tag"), py::arg("now") = -1, py::arg("t0_ns") = 0)
      .def("submit_tx_many", [](PyServe& s, py::list items, py::list tags, int64_t now, py::list t0s) {
        const size_t n = items.size();
        if (tags.size() != n || (t0s.size() && t0s.size() != n)) throw std::runtime_error("submit_tx_many: lengths");
        std::vector<std::pair<const char*, size_t>> bufs(n);
        std::vector<uint64_t> tg(n);
        std::vector<int64_t> t0(n, 0);
        for (size_t k = 0; k < n; ++k) {
          char* p; py::ssize_t ln;
          if (PYBIND11_BYTES_AS_STRING_AND_SIZE(items[k].ptr(), &p, &ln) != 0) throw std::runtime_error("bytes expected");
          bufs[k] = {p, size_t(ln)};
          tg[k] = tags[k].cast<uint64_t>();
          if (t0s.size()) t0[k] = t0s[k].cast<int64_t>();
        }
        py::gil_scoped_release rel;
        for (size_t k = 0; k < n; ++k) s.core->submit_tx(bufs[k].first, bufs[k].second, tg[k], now, t0[k]);
      }, py::arg("items"), py::arg("tags"), py::arg("now") = -1, py::arg("t0s") = py::list())
      .def("poll", [](PyServe& s, size_t max, int64_t timeout_us) {
        std::vector<ServeCore::Done> out;
        {
          py::gil_scoped_release rel;
          s.core->poll(out, max, timeout_us);
        }
        py::list l;
        for (auto& d : out) {
          if (d.err.empty()) l.append(py::make_tuple(d.tag, py::bytes(d.bytes), py::none()));
          else l.append(py::make_tuple(d.tag, py::none(), py::str(d.err)));
        }
        return l;
      }, py::arg("max") = 4096, py::arg("timeout_us") = 1000)
      .def("pause", [](PyServe& s) { py::gil_scoped_release rel; s.core->pause(); })
      .def("resume", [](PyServe& s) { s.core->resume(); })
      .def("set_device", [](PyServe& s, py::object dev) {
        const IgpDeviceOps* ops = device_ops_of(dev);
        s.core->set_device(ops);
        s.dev = dev;
      })
      .def("stop", [](PyServe& s) { py::gil_scoped_release rel; s.core->stop(); })
      .def("abort", [](PyServe& s) { py::gil_scoped_release rel; s.core->abort(); })
      .def("set_links", [](PyServe& s, std::shared_ptr<LinkIndex> l) { s.core->set_links(std::move(l)); })
      .def("set_audit", [](PyServe& s, std::shared_ptr<AuditRing> a) { s.core->set_audit(std::move(a)); })
      .def("set_model_version", [](PyServe& s, int v) { s.core->set_model_version(v); })
      .def("pending_items", [](PyServe& s) { return s.core->pending_items(); })
      .def_property_readonly("issued", [](const PyServe& s) { return s.core->issued(); })
      .def_property_readonly("seq", [](const PyServe& s) { return s.core->seq(); })
      .def_property_readonly("late_steps", [](const PyServe& s) { return s.core->late_steps(); })
      .def_property_readonly("world", [](const PyServe& s) { return s.core->world(); })
      .def("stats", [](PyServe& s, bool reset) {
        ServeStats t = s.core->stats(reset);
        py::dict d;
        d["items"] = t.items; d["rows"] = t.rows; d["steps"] = t.steps; d["empty_steps"] = t.empty_steps;
        d["unary"] = t.unary; d["parse_ns"] = t.parse_ns; d["resolve_ns"] = t.resolve_ns; d["pack_ns"] = t.pack_ns;
        d["device_ns"] = t.device_ns; d["copy_ns"] = t.copy_ns; d["serialize_ns"] = t.serialize_ns;
        d["submit_ns"] = t.submit_ns; d["wait_errors"] = t.wait_errors; d["max_step_rows"] = t.max_step_rows;
        d["release_ns"] = t.release_ns; d["slot_wait_ns"] = t.slot_wait_ns; d["rows_wait_ns"] = t.rows_wait_ns;
        d["slot_waits"] = t.slot_waits; d["slot_wait_inflight"] = t.slot_wait_inflight;
        d["inplace_steps"] = t.inplace_steps; d["packed_steps"] = t.packed_steps;
        d["rowbufs"] = t.rowbufs; d["rowbufs_free"] = t.rowbufs_free;
        d["actions"] = py::make_tuple(t.actions[0], t.actions[1], t.actions[2], t.actions[3]);
        py::list dl;
        for (int k = 0; k < 11; ++k) dl.append(t.deciles[k]);
        d["deciles"] = dl;
        d["ml_high"] = t.ml_high; d["blacklisted"] = t.blacklisted; d["scored"] = t.scored;
        return d;
      }, py::arg("reset") = false)
      .def_static("now_ns", &ServeCore::now_ns)
      .def_static("last_timings", []() {  // this thread's last score_batch call, ns per stage
        const CallTimings& t = last_timings_tl();
        return py::make_tuple(t.parse, t.resolve, t.queue, t.device, t.serialize, t.total, t.rows, t.seq_first,
                              t.seq_last);
      });

  // ---- account RPCs (acct_core.h): PredictLTV / GetPlayerSegment / CheckBonusAbuse
  m.attr("RPC_LTV") = int(RPC_LTV);
  m.attr("RPC_SEGMENT") = int(RPC_SEGMENT);
  m.attr("RPC_ABUSE") = int(RPC_ABUSE);
  py::class_<CpuLtvDevice, std::shared_ptr<CpuLtvDevice>>(m, "CpuLtvDevice")
      .def(py::init([](py::array rows, py::array present, py::object ext, py::object model, std::string in_name,
                       std::string out_name, int width, int depth, int cap) {
             // the arrays stay owned by the caller (engine/ltv.py PlayerTable), which keeps them alive
             auto r = py::array_t<float, py::array::c_style>::ensure(rows);
             auto pr = py::array_t<uint8_t, py::array::c_style>::ensure(present);
             if (!r || !pr || r.ndim() != 2 || r.shape(1) != 25 || pr.size() != r.shape(0))
               throw std::runtime_error("CpuLtvDevice: rows [C, 25] f32 and present [C] (bool / uint8) expected");
             if (static_cast<const void*>(r.data()) != rows.data() || static_cast<const void*>(pr.data()) != present.data())
               throw std::runtime_error("CpuLtvDevice: the tables must be C-contiguous (no copies)");
             const float* ep = nullptr;
             int ew = 0;
             if (!ext.is_none()) {
               auto e = py::array_t<float, py::array::c_style>::ensure(ext);
               if (!e || static_cast<const void*>(e.data()) != ext.cast<py::array>().data() || e.ndim() != 2 ||
                   e.shape(0) != r.shape(0))
                 throw std::runtime_error("CpuLtvDevice: ext [C, w] f32, C-contiguous");
               ep = e.data();
               ew = int(e.shape(1));
             }
             std::shared_ptr<exec::Executor> ex;
             if (!model.is_none()) ex = model.cast<std::shared_ptr<exec::Executor>>();
             return std::make_shared<CpuLtvDevice>(r.data(), pr.data(), ep, ew, int64_t(r.shape(0)), ex, in_name,
                                                   out_name, width, depth, cap);
           }),
           py::arg("rows"), py::arg("present"), py::arg("ext"), py::arg("model"), py::arg("in_name") = "input",
           py::arg("out_name") = "output", py::arg("width") = 0, py::arg("depth") = 2, py::arg("cap") = 4096)
      .def("model_ops", [](const CpuLtvDevice& d) { return reinterpret_cast<uintptr_t>(d.ops()); });
  py::class_<CpuAbuseDevice, std::shared_ptr<CpuAbuseDevice>>(m, "CpuAbuseDevice")
      .def(py::init<std::shared_ptr<CpuScorer>, std::shared_ptr<exec::Executor>, std::string, std::string, int, int,
                    std::string>(),
           py::arg("scorer"), py::arg("model"), py::arg("in_name") = "input", py::arg("out_name") = "output",
           py::arg("depth") = 2, py::arg("cap") = 4096, py::arg("lens_name") = "")
      .def("model_ops", [](const CpuAbuseDevice& d) { return reinterpret_cast<uintptr_t>(d.ops()); });

  py::class_<PyAcct, std::shared_ptr<PyAcct>>(m, "AcctRouter")
      .def(py::init([](std::vector<std::shared_ptr<AccountIndex>> idx, int rank, std::string mailbox, bool create) {
             auto p = std::make_shared<PyAcct>();
             py::gil_scoped_release rel;
             p->router = std::make_shared<AcctRouter>(std::move(idx), rank, mailbox, create);
             return p;
           }),
           py::arg("indexes"), py::arg("rank") = 0, py::arg("mailbox") = "", py::arg("create") = false)
      .def("attach", [](PyAcct& a, py::object dev, int max_wait_us, int64_t timeout_us, int finishers) {
        AcctCore::Options o;
        o.max_wait_us = max_wait_us;
        o.timeout_us = timeout_us;
        o.finishers = finishers;
        const IgpModelOps* ops = model_ops_of(dev);
        a.devs.push_back(dev);
        py::gil_scoped_release rel;
        a.router->attach(ops, o);
      }, py::arg("device"), py::arg("max_wait_us") = 200, py::arg("timeout_us") = -1, py::arg("finishers") = 2)
      .def("set_device", [](PyAcct& a, py::object dev) {
        const IgpModelOps* ops = model_ops_of(dev);
        a.devs.push_back(dev);  // the old table may still be read by a step in flight: keep it
        py::gil_scoped_release rel;
        a.router->set_device(ops->kind, ops);
      })
      .def("pause", [](PyAcct& a) {
        py::gil_scoped_release rel;
        a.router->pause();
      })
      .def("resume", [](PyAcct& a) { a.router->resume(); })
      .def("set_links", [](PyAcct& a, std::shared_ptr<LinkIndex> l) { a.router->set_links(std::move(l)); })
      .def("set_abuse", [](PyAcct& a, int max_devices, int max_ips, int max_tx_per_minute, double threshold,
                           std::vector<double> weights, int linked_limit, int64_t link_wait_us) {
        AbuseParams p;
        p.max_devices_per_day = max_devices;
        p.max_ips_per_day = max_ips;
        p.max_tx_per_minute = max_tx_per_minute;
        p.threshold = threshold;
        if (weights.size() != 7) throw std::runtime_error("set_abuse: 7 signal weights");
        for (int k = 0; k < 7; ++k) p.w[k] = weights[size_t(k)];
        p.linked_limit = linked_limit;
        p.link_wait_us = link_wait_us;
        a.router->set_abuse(p);
      }, py::arg("max_devices"), py::arg("max_ips"), py::arg("max_tx_per_minute"), py::arg("threshold"),
         py::arg("weights"), py::arg("linked_limit") = 16, py::arg("link_wait_us") = AbuseParams().link_wait_us)
      .def("serves", [](PyAcct& a, int rpc) { return a.router->serves(uint8_t(rpc)); })
      .def("submit", [](PyAcct& a, int rpc, py::bytes data, uint64_t tag, int64_t t0_ns, int64_t now) {
        char* p; py::ssize_t n;
        PYBIND11_BYTES_AS_STRING_AND_SIZE(data.ptr(), &p, &n);
        a.router->submit(uint8_t(rpc), p, size_t(n), tag, t0_ns, now);
      }, py::arg("rpc"), py::arg("data"), py::arg("tag"), py::arg("t0_ns") = 0, py::arg("now") = -1)
      .def("submit_many", [](PyAcct& a, int rpc, py::list items, py::list tags, int64_t now) {
        const size_t n = items.size();
        if (tags.size() != n) throw std::runtime_error("submit_many: lengths");
        std::vector<std::string> bufs(n);
        std::vector<uint64_t> tg(n);
        for (size_t k = 0; k < n; ++k) {
          bufs[k] = items[k].cast<std::string>();
          tg[k] = tags[k].cast<uint64_t>();
        }
        py::gil_scoped_release rel;
        const int64_t t0 = ServeCore::now_ns();
        for (size_t k = 0; k < n; ++k) a.router->submit(uint8_t(rpc), bufs[k].data(), bufs[k].size(), tg[k], t0, now);
      }, py::arg("rpc"), py::arg("items"), py::arg("tags"), py::arg("now") = -1)
      .def("poll", [](PyAcct& a, size_t max, int64_t timeout_us) {
        std::vector<AcctRouter::Done> out;
        {
          py::gil_scoped_release rel;
          a.router->poll(out, max, timeout_us);
        }
        py::list l;
        for (auto& d : out) {
          if (d.err.empty()) l.append(py::make_tuple(d.tag, py::bytes(d.bytes), py::none()));
          else l.append(py::make_tuple(d.tag, py::none(), py::str(d.err)));
        }
        return l;
      }, py::arg("max") = 4096, py::arg("timeout_us") = 1000)
      // in-process closed-loop load (bench.py --config cfg4|cfg5 --scope serving): `n` calls
      // cycling over `payloads`, at most `inflight` outstanding, submitted by `threads` threads
      // (call i by thread i % threads) and answered on this thread, all without the GIL. Returns
      // per-call latency (submit -> answer, ns; -1 for an error), the error count, the cold-path
      // count ("cold: " replies) and the elapsed seconds.
      .def("drive", [](PyAcct& a, int rpc, py::list payloads, int64_t n, int64_t inflight, int64_t now, int threads) {
        const size_t np_ = payloads.size();
        if (np_ == 0 || n <= 0 || inflight <= 0 || threads < 1 || threads > 64)
          throw std::runtime_error("drive: payloads, n and inflight > 0, 1..64 threads");
        std::vector<std::string> bufs(np_);
        for (size_t k = 0; k < np_; ++k) bufs[k] = payloads[k].cast<std::string>();
        std::vector<int64_t> t_sub(size_t(n), 0);
        py::array_t<int64_t> lat(n);
        int64_t* L = lat.mutable_data();
        int64_t got = 0, errors = 0, cold = 0;
        double elapsed = 0;
        {
          py::gil_scoped_release rel;
          const int T = threads;
          const int64_t cap = std::max<int64_t>(1, inflight / T);
          std::atomic<bool> abort{false};
          const int64_t t0 = ServeCore::now_ns();
          if (T == 1) {
            // one thread submits every free window slot, then polls (no hand-off between a
            // submitting and a polling thread: the submitter's back-off sleeps left the window
            // part-empty, cfg5 1.92 -> 1.18 M checks/s)
            int64_t sent = 0, idle_since = 0;
            std::vector<AcctRouter::Done> out;
            while (got < n) {
              const int64_t room = std::min<int64_t>(n - sent, inflight - (sent - got));
              for (int64_t k = 0; k < room; ++k, ++sent) {
                const std::string& b = bufs[size_t(sent) % np_];
                const int64_t ts = ServeCore::now_ns();
                t_sub[size_t(sent)] = ts;
                a.router->submit(uint8_t(rpc), b.data(), b.size(), uint64_t(sent), ts, now);
              }
              out.clear();
              a.router->poll(out, size_t(std::max<int64_t>(inflight, 1024)), 2000);
              const int64_t tr = ServeCore::now_ns();
              if (out.empty()) {
                if (!idle_since) idle_since = tr;
                if (tr - idle_since > 60000000000LL) break;  // nothing answered for a minute: give up
                continue;
              }
              idle_since = 0;
              for (auto& d : out) {
                const size_t i = size_t(d.tag);
                if (i >= size_t(n)) continue;
                if (!d.err.empty()) {
                  ++errors;
                  if (d.err.compare(0, std::strlen(kColdPrefix), kColdPrefix) == 0) ++cold;
                  L[got++] = -1;
                } else {
                  L[got++] = tr - t_sub[i];
                }
              }
            }
            elapsed = double(ServeCore::now_ns() - t0) / 1e9;
            for (int64_t k = got; k < n; ++k) L[k] = -1;
            errors += n - got;
          }
          if (T > 1) {
            // T submitting threads, each with its own window of inflight / T calls. The answers
            // come back through the router's sink on the cores' finisher threads (no polling
            // thread, no queue hand-off), which record the latency and reopen the submitter's
            // window; a submitter yields on a full window instead of sleeping (VERDICT r5 item
            // 5: the sleeping submitters of round 5 left the window part-empty). The state is
            // shared with the sink, so an answer that arrives after a give-up touches nothing
            // freed.
            struct Shared {
              std::vector<int64_t> t_sub, lat;
              std::vector<std::atomic<int64_t>> done;
              std::atomic<int64_t> got{0}, errors{0}, cold{0};
              int64_t n;
              int T;
              Shared(int64_t n_, int T_) : t_sub(size_t(n_), 0), lat(size_t(n_), -1), done(size_t(T_)), n(n_), T(T_) {
                for (auto& d : done) d.store(0);
              }
            };
            auto sh = std::make_shared<Shared>(n, T);
            auto prev = a.router->sink();
            a.router->set_sink([sh](std::vector<AcctRouter::Done>&& outs) {
              // one atomic add per submitter and one for the total per delivered range, not per
              // answer (the finishers' per-answer adds on shared lines cost more than the answers)
              const int64_t tr = ServeCore::now_ns();
              int64_t per[64] = {0};
              int64_t n_ok = 0;
              for (auto& d : outs) {
                const uint64_t i = d.tag & ~AcctRouter::kSinkTag;
                if (i >= uint64_t(sh->n)) continue;
                if (!d.err.empty()) {
                  sh->errors.fetch_add(1);
                  if (d.err.compare(0, std::strlen(kColdPrefix), kColdPrefix) == 0) sh->cold.fetch_add(1);
                  sh->lat[size_t(i)] = -1;
                } else {
                  sh->lat[size_t(i)] = tr - sh->t_sub[size_t(i)];
                }
                ++per[i % uint64_t(sh->T)];
                ++n_ok;
              }
              for (int j = 0; j < sh->T; ++j)
                if (per[j]) sh->done[size_t(j)].fetch_add(per[j], std::memory_order_release);
              if (n_ok) sh->got.fetch_add(n_ok, std::memory_order_acq_rel);
            });
            // each submitter hands its calls over in batches of up to kBatch (one queue-lock
            // acquisition per batch: four threads taking the lock per call ran slower than one)
            constexpr int64_t kBatch = 64;
            std::vector<std::thread> subs;
            for (int j = 0; j < T; ++j) {
              subs.emplace_back([&, j, sh] {
                int64_t sent = 0;  // calls j, j + T, j + 2T, ... of this thread
                std::vector<std::string_view> dv;
                std::vector<uint64_t> tg;
                std::vector<int64_t> ts;
                for (int64_t i = j; i < n && !abort.load(std::memory_order_relaxed);) {
                  int64_t room;
                  while ((room = cap - (sent - sh->done[size_t(j)].load(std::memory_order_acquire))) <= 0) {
                    if (abort.load(std::memory_order_relaxed)) return;
                    std::this_thread::yield();
                  }
                  dv.clear();
                  tg.clear();
                  ts.clear();
                  const int64_t t = ServeCore::now_ns();
                  for (int64_t k = 0; k < std::min(room, kBatch) && i < n; ++k, i += T) {
                    const std::string& b = bufs[size_t(i) % np_];
                    sh->t_sub[size_t(i)] = t;
                    dv.emplace_back(b.data(), b.size());
                    tg.push_back(AcctRouter::kSinkTag | uint64_t(i));
                    ts.push_back(t);
                  }
                  a.router->submit_many(uint8_t(rpc), dv.data(), tg.data(), ts.data(), dv.size(), now);
                  sent += int64_t(dv.size());
                }
              });
            }
            int64_t last = -1, idle_since = ServeCore::now_ns();
            while (sh->got.load(std::memory_order_acquire) < n) {
              std::this_thread::sleep_for(std::chrono::microseconds(200));
              const int64_t g = sh->got.load(std::memory_order_acquire), tr = ServeCore::now_ns();
              if (g != last) {
                last = g;
                idle_since = tr;
              } else if (tr - idle_since > 60000000000LL) {  // nothing answered for a minute: give up
                abort.store(true);
                break;
              }
            }
            for (auto& t : subs) t.join();
            elapsed = double(ServeCore::now_ns() - t0) / 1e9;
            a.router->set_sink(prev);
            got = sh->got.load();
            errors = sh->errors.load() + (n - got);
            cold = sh->cold.load();
            std::memcpy(L, sh->lat.data(), sizeof(int64_t) * size_t(n));
          }
        }
        py::dict r;
        r["latency_ns"] = lat;
        r["errors"] = errors;
        r["cold"] = cold;
        r["elapsed"] = elapsed;
        return r;
      }, py::arg("rpc"), py::arg("payloads"), py::arg("n"), py::arg("inflight") = 8192, py::arg("now") = -1,
         py::arg("threads") = 1)
      .def("stop", [](PyAcct& a) {
        py::gil_scoped_release rel;
        a.router->stop();
      })
      .def("unlink_shared", [](PyAcct& a) { a.router->unlink_shared(); })
      .def("stats", [](PyAcct& a, int kind, bool reset) { return acct_stats_dict(a.router->stats(kind, reset)); },
           py::arg("kind"), py::arg("reset") = false)
      .def_property_readonly("remote_out", [](const PyAcct& a) { return a.router->remote_out(); })
      .def_property_readonly("remote_expired", [](const PyAcct& a) { return a.router->remote_expired(); })
      .def_property_readonly("reply_oversize", [](const PyAcct& a) { return a.router->reply_oversize(); })
      .def_property_readonly("world", [](const PyAcct& a) { return a.router->world(); })
      .def_property_readonly("rank", [](const PyAcct& a) { return a.router->rank(); })
      .def_property("remote_timeout_us", [](const PyAcct& a) { return a.router->remote_timeout_us; },
                    [](PyAcct& a, int64_t v) { a.router->remote_timeout_us = v; });
}
