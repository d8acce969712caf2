"""
Layered arithmetic circuit for the GKR protocol, with the reference's builder interface
(python/zksnake/arithmetization/layered_circuit.py:4-104): `LayeredCircuit(inputs)`, `add_layer`, `add_gate` / `add` / `mul`,
`get_wire_label`, `evaluate`.

Layer 0 is the inputs; layer j >= 1 is a list of gates (type, in1, in2) over the wires of layer j-1.  There is ONE numbering of
wires: wire t of layer j is the output of gate t of layer j, wire t of layer 0 is `inputs[t]`, and a wire that nothing reads
keeps its slot.  (The reference numbers a layer's wires by first use in the layer above and the same layer's gates by
position; the two disagree as soon as the layer above reads wires in another order.  `get_wire_label()` still returns the
reference's lists, as data about names; nothing here indexes by them.)

Beyond the reference: `from_arrays` takes the gates of a circuit too large to name wire by wire, and `compile()` gives the
device form the GKR prover works on -- per layer the gate arrays and the two CSRs of subprotocol/gkr.py, built once with numpy.
"""

import numpy as np

from .. import _native as N
from ..device import DeviceBuffer
from ..spmv import ITEM, LONG_ROW, long_row_items

ADD, MUL = 0, 1
_TYPES = {"ADD": ADD, "MUL": MUL}

assert LONG_ROW == N.GKR_LONG_ROW, "the GKR passes split rows where the sparse matrix product does"


def num_vars(n):
    """variables of a layer of n wires: max(1, ceil(log2 n))"""
    return max(1, (int(n) - 1).bit_length())


class GateCsr:
    """The gates of one layer grouped by one of their inputs (`rows`), the other input beside them: device arrays row_ptr,
    gate, other, types and the long-row work items of spmv.long_row_items.  The host copies stay for tests and tools."""

    def __init__(self, log_rows, rows, other, types):
        n_rows = 1 << log_rows
        order = np.argsort(rows, kind="stable").astype(np.uint32)
        self.log_rows = log_rows
        self.n_entries = int(rows.shape[0])
        self.row_ptr = np.zeros(n_rows + 1, dtype=np.uint32)
        np.cumsum(np.bincount(rows, minlength=n_rows), out=self.row_ptr[1:])
        self.gate = order
        self.other = np.ascontiguousarray(other[order], dtype=np.uint32)
        self.types = np.ascontiguousarray(types[order], dtype=np.uint8)
        self.long_rows, self.item_ptr, self.items = long_row_items(self.row_ptr, LONG_ROW, ITEM)
        self.n_long, self.n_items = int(self.long_rows.shape[0]), int(self.items.shape[0])
        self.d_row_ptr = DeviceBuffer.from_numpy(self.row_ptr)
        self.d_gate = DeviceBuffer.from_numpy(self.gate)
        self.d_other = DeviceBuffer.from_numpy(self.other)
        self.d_types = DeviceBuffer.from_numpy(self.types)
        if self.n_long:
            self.d_long_rows = DeviceBuffer.from_numpy(self.long_rows)
            self.d_item_ptr = DeviceBuffer.from_numpy(self.item_ptr)
            self.d_items = DeviceBuffer.from_numpy(self.items)
            self.d_partials = DeviceBuffer(2 * self.n_items * 32)

    def args(self):
        """the CSR part of the argument list of zk_gkr_phase1_dev / zk_gkr_phase2_dev"""
        long_part = (self.n_long, self.d_long_rows.ptr, self.d_item_ptr.ptr, self.n_items, self.d_items.ptr, self.d_partials.ptr) \
            if self.n_long else (0, None, None, 0, None, None)
        return (self.log_rows, self.n_entries, self.d_row_ptr.ptr, self.d_gate.ptr, self.d_other.ptr, self.d_types.ptr) + long_part


class CompiledLayer:
    """layer j >= 1 on the device: n gates over the n_prev wires below; k, k_prev variables; gate arrays; the CSR by in1
    (phase 1) and by in2 (phase 2)"""

    def __init__(self, n_prev, types, in1, in2, j=0):
        types, in1, in2 = _check_layer(j, n_prev, types, in1, in2)
        self.n, self.n_prev = int(types.shape[0]), int(n_prev)
        self.k, self.k_prev = num_vars(self.n), num_vars(self.n_prev)
        self.types, self.in1, self.in2 = types, in1, in2
        self.d_types = DeviceBuffer.from_numpy(types)
        self.d_in1 = DeviceBuffer.from_numpy(in1)
        self.d_in2 = DeviceBuffer.from_numpy(in2)
        self.by_b = GateCsr(self.k_prev, in1, in2, types)
        self.by_c = GateCsr(self.k_prev, in2, in1, types)


def _check_layer(j, n_prev, types, in1, in2):
    """the one bounds check of the gathers: every kernel trusts these arrays"""
    types = np.ascontiguousarray(types, dtype=np.uint8).reshape(-1)
    if np.asarray(in1).shape != types.shape or np.asarray(in2).shape != types.shape:
        raise ValueError(f"layer {j}: types, in1 and in2 differ in length")
    if types.shape[0] == 0:
        raise ValueError(f"layer {j} has no gate")
    if types.shape[0] > 1 << N.GKR_MAX_LOG or n_prev > 1 << N.GKR_MAX_LOG:
        raise ValueError(f"layer {j}: at most 2^{N.GKR_MAX_LOG} wires and gates per layer")
    if types.max() > MUL:
        raise ValueError(f"layer {j}: a gate type is neither ADD (0) nor MUL (1)")
    wide1, wide2 = np.asarray(in1).astype(np.int64).reshape(-1), np.asarray(in2).astype(np.int64).reshape(-1)
    for wide in (wide1, wide2):
        if wide.min() < 0 or wide.max() >= n_prev:
            raise ValueError(f"layer {j}: a gate reads wire {int(wide.max() if wide.max() >= n_prev else wide.min())} "
                             f"of a layer of {n_prev} wires")
    return types, wide1.astype(np.uint32), wide2.astype(np.uint32)


class LayeredCircuit:
    def __init__(self, inputs):
        self.inputs = list(inputs)
        if not self.inputs:
            raise ValueError("a circuit needs an input")
        if len(set(self.inputs)) != len(self.inputs):
            raise ValueError("input names repeat")
        self.layers = [[]]                     # the reference's attribute: per layer a list of (type, in1, in2, out) by name
        self.named = True
        self._arrays = None                    # from_arrays: [(types, in1, in2), ..] instead of names
        self._index = {name: t for t, name in enumerate(self.inputs)}   # wires of the layer below the current one
        self._used = set(self.inputs)
        self._compiled = None

    @classmethod
    def from_arrays(cls, n_inputs, layers):
        """n_inputs wires in layer 0 and, per layer, (types u8: 0 ADD / 1 MUL, in1 u32, in2 u32) indexing the layer below.
        Wires have no names: inputs and outputs travel as sequences in wire order."""
        self = cls(range(int(n_inputs)))
        self.named, self.layers, self._index, self._used = False, None, None, None
        self._arrays, n_prev = [], int(n_inputs)
        for j, (types, in1, in2) in enumerate(layers, start=1):
            self._arrays.append(_check_layer(j, n_prev, types, in1, in2))
            n_prev = self._arrays[-1][0].shape[0]
        if not self._arrays:
            raise ValueError("a circuit needs a layer")
        return self

    # -- the reference's builder --
    def add_layer(self):
        """close the current layer (when it has a gate) and start the next one over its outputs"""
        self._need_names()
        if self.layers[-1]:
            self._index = {gate[3]: t for t, gate in enumerate(self.layers[-1])}
            self.layers.append([])

    def add_gate(self, gate_type, input1, input2, output):
        self._need_names()
        if gate_type not in _TYPES:
            raise ValueError("Invalid gate type")
        if input1 not in self._index or input2 not in self._index:
            raise ValueError(f"Gate inputs {input1}, {input2} must be outputs of the previous layer, or inputs in the first layer")
        if output in self._used:
            raise ValueError(f"Variable already used: {output}")
        self._used.add(output)
        self.layers[-1].append((gate_type, input1, input2, output))
        self._compiled = None

    def add(self, input1, input2, output):
        self.add_gate("ADD", input1, input2, output)

    def mul(self, input1, input2, output):
        self.add_gate("MUL", input1, input2, output)

    def _need_names(self):
        if not self.named:
            raise TypeError("a circuit made by from_arrays has no named wires")

    def get_wire_label(self):
        """per layer the names its gates read, in order of first use, then the names of the last layer's outputs: the
        reference's lists.  Data about names only -- see the module docstring."""
        self._need_names()
        labels = []
        for layer in self._closed_layers():
            labels.append(list(dict.fromkeys(name for _, in1, in2, _ in layer for name in (in1, in2))))
        labels.append([gate[3] for gate in self._closed_layers()[-1]])
        return labels

    def _closed_layers(self):
        layers = self.layers if self.layers[-1] else self.layers[:-1]
        if not layers:
            raise ValueError("the circuit has no gate")
        return layers

    # -- the one numbering --
    def gate_arrays(self):
        """[(types u8, in1 u32, in2 u32), ..] for layers 1 .. d, indices into the layer below; checked"""
        if self._arrays is not None:
            return self._arrays
        out, index = [], {name: t for t, name in enumerate(self.inputs)}
        for j, layer in enumerate(self._closed_layers(), start=1):
            types = np.array([_TYPES[g[0]] for g in layer], dtype=np.uint8)
            in1 = np.array([index[g[1]] for g in layer], dtype=np.int64)
            in2 = np.array([index[g[2]] for g in layer], dtype=np.int64)
            out.append(_check_layer(j, len(index), types, in1, in2))
            index = {g[3]: t for t, g in enumerate(layer)}
        return out

    def output_names(self):
        self._need_names()
        return [gate[3] for gate in self._closed_layers()[-1]]

    def evaluate(self, input_map, modulus):
        """every wire's value, on the host with Python integers: [inputs, layer 1, .., layer d], dicts by name for a named
        circuit (`input_map` a dict over exactly the inputs), lists in wire order otherwise"""
        if self.named:
            if set(input_map.keys()) != set(self.inputs):
                raise ValueError("Insufficient input values are supplied")
            values = [int(input_map[name]) % modulus for name in self.inputs]
        else:
            values = [int(v) % modulus for v in input_map]
            if len(values) != len(self.inputs):
                raise ValueError("Insufficient input values are supplied")
        rows = [values]
        for types, in1, in2 in self.gate_arrays():
            values = [(values[b] * values[c] if t else values[b] + values[c]) % modulus
                      for t, b, c in zip(types.tolist(), in1.tolist(), in2.tolist())]
            rows.append(values)
        if not self.named:
            return rows
        names = [self.inputs] + [[g[3] for g in layer] for layer in self._closed_layers()]
        return [dict(zip(n, r)) for n, r in zip(names, rows)]

    def compile(self, p=None):
        """[CompiledLayer for layers 1 .. d], cached until a gate is added.  The device form holds indices only, so it is the
        same for every field; `p` is accepted for callers that think of a circuit over a field."""
        if self._compiled is None:
            n_prev, out = len(self.inputs), []
            for j, (types, in1, in2) in enumerate(self.gate_arrays(), start=1):
                out.append(CompiledLayer(n_prev, types, in1, in2, j))
                n_prev = out[-1].n
            self._compiled = out
        return self._compiled
