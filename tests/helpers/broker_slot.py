"""A broker client's own shared-memory slot, seen as the resident kernel sees it in direct serving (moira_amd/csrc/mpb_broker.cpp:
BrkSlot): the door word, the kernel's result line, the request's 64 bytes of parameters and the packed row.  For the tests that post
a request by hand -- forged parameters, a forged length -- to the slot of a client they own."""
import ctypes as C
import time

import numpy as np

DOOR_OFF, DONE_OFF, NS_OFF, EE_OFF, PASS_OFF, PRM_OFF, ROW_OFF = 320, 384, 388, 392, 400, 448, 512


class _Handle(C.Structure):                  # the client handle starts with the Mapping {base, bytes}, then the slot index
    _fields_ = [("base", C.c_void_p), ("bytes", C.c_size_t), ("slot", C.c_int)]


class DirectSlot:
    def __init__(self, cl, row_bytes=2048):
        hd = _Handle.from_address(cl.h.value)
        raw = (C.c_char * hd.bytes).from_address(hd.base)
        n_slots, slot_bytes = (int(v) for v in np.frombuffer(raw, np.int32, 2, 8))
        so = hd.bytes - n_slots * slot_bytes + hd.slot * slot_bytes
        self.index = int(hd.slot)
        self.door = np.frombuffer(raw, np.uint64, 1, so + DOOR_OFF)
        self.done = np.frombuffer(raw, np.uint32, 1, so + DONE_OFF)
        self.d_ns = np.frombuffer(raw, np.int32, 1, so + NS_OFF)
        self.d_ee = np.frombuffer(raw, np.float64, 1, so + EE_OFF)
        self.d_pass = np.frombuffer(raw, np.uint8, 1, so + PASS_OFF)
        self.prm = np.frombuffer(raw, np.uint8, 64, so + PRM_OFF)
        self.row = np.frombuffer(raw, np.uint8, row_bytes, so + ROW_OFF)

    def served_directly(self):
        """After an honest call: did the kernel itself answer it in the slot (the token of the door word is the token served)?"""
        return int(self.door[0]) != 0 and int(self.done[0]) == int(self.door[0]) & 0xffffffff

    def post(self, length, blob=None, timeout=10.0):
        """The next token with `length` (and, when given, 64 bytes of parameters) for the row that lies in the slot ->
        (ee, ns, pass) as the kernel wrote them."""
        if blob is not None:
            self.prm[:] = np.frombuffer(blob, np.uint8)
        tok = (int(self.door[0]) & 0xffffffff) + 1
        self.door[0] = (int(length) << 32) | tok
        t0 = time.time()
        while int(self.done[0]) != tok and time.time() - t0 < timeout:
            time.sleep(0.0005)
        assert int(self.done[0]) == tok
        return float(self.d_ee[0]), int(self.d_ns[0]), int(self.d_pass[0])
