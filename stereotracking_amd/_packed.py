"""The host scaffold of a device evaluator or post-processor ("One packed call"): host tables
side by side in one buffer and ONE upload, the outputs side by side in a second buffer, the stage entries on the
caller's current stream, ONE wait and ONE copy back, the timing dict.

    call = PackedCall('the MOT evaluation', 'csrc/mot_eval.hip', device, timing, LAUNCHES)
    call.upload(dict(rows=..., offsets=...))
    call.outputs([('status', (8,), np.int32), ...])
    call.bind(args)
    call.workspace(args, call.workspace_bytes('st_..._workspace_bytes', args))
    with call.stages():
        call.launch('st_...', C.byref(args))
    host = call.fetch()                       # {output name: host view}
    return result, call.timing_dict()

The caller names every export as a string literal; it is looked up on the loaded handle when it is called.
"""
import contextlib
import ctypes as C
import time

import numpy as np
import torch

from . import _lib


class _Layout:
    """Arrays side by side in one byte buffer, every one at a multiple of 256 bytes."""

    def __init__(self, specs=()):
        self.items, self.size = {}, 0
        for name, shape, dtype in specs:
            self.add(name, shape, dtype)

    def add(self, name, shape, dtype):
        dtype = np.dtype(dtype)
        n = int(np.prod(shape, dtype=np.int64)) * dtype.itemsize
        self.items[name] = (self.size, tuple(int(v) for v in shape), dtype)
        self.size += (n + 255) // 256 * 256 + 256

    def view(self, buf, name):
        off, shape, dtype = self.items[name]
        n = int(np.prod(shape, dtype=np.int64))
        return buf[off:off + n * dtype.itemsize].view(dtype).reshape(shape)

    def fill(self, arrays):
        """A zeroed host buffer of the layout's size that holds `arrays` (name -> array)."""
        buf = np.zeros(self.size, np.uint8)
        for k, v in arrays.items():
            self.view(buf, k)[...] = v
        return buf

    def bind(self, args, base, names=None):
        """args.<name> = base + the offset of <name>, for `names` (default: every array of the layout)."""
        for k in self.items if names is None else names:
            setattr(args, k, C.c_void_p(base + self.items[k][0]))


def _device_view(layout, buf, name):
    """_Layout.view for the device copy of the buffer (a uint8 tensor)."""
    off, shape, dtype = layout.items[name]
    n = int(np.prod(shape, dtype=np.int64))
    return buf[off:off + n * dtype.itemsize].view(getattr(torch, dtype.name)).view(shape)


class PackedCall:
    """One call of a device entry; see the module docstring.  what / source: the entry's name and its HIP file, for the
    messages; launches: the calling module's LAUNCHES counter.  The clock of the timing dict starts here."""

    def __init__(self, what, source, device, timing, launches):
        self.t_start = time.perf_counter()
        if not torch.cuda.is_available():
            raise RuntimeError(f'the device backend of {what} runs on the HIP path only ({source}) and no CUDA (ROCm) '
                               f'device is available; use backend=\'host\'')
        self.lib = _lib.load()
        dev = torch.device(device) if device is not None else torch.device('cuda')
        if dev.type != 'cuda':
            raise RuntimeError(f'the device backend of {what} needs a CUDA (ROCm) device, got {dev}')
        self.dev = dev if dev.index is not None else torch.device('cuda', torch.cuda.current_device())
        self.timing, self.launches, self.events, self.interval = timing, launches, [], None

    def upload(self, host_in):
        """The one upload of the host arrays (name -> array)."""
        self.lin = _Layout((k, v.shape, v.dtype) for k, v in host_in.items())
        self.hbuf = self.lin.fill(host_in)        # kept until the call object goes: freeing it is not part of the timed upload
        self.t_prep = time.perf_counter()
        self.dbuf = torch.from_numpy(self.hbuf).to(self.dev)

    def outputs(self, specs, zero=False):
        """The output buffer of (name, shape, dtype) specs; not zeroed unless `zero`: the stages write what is read."""
        self.lout = _Layout(specs)
        self.obuf = (torch.zeros if zero else torch.empty)(self.lout.size, dtype=torch.uint8, device=self.dev)

    def bind(self, args, inputs=None, outputs=None):
        """Sets the pointers of the uploaded arrays and the outputs on the args struct (default: all of them)."""
        self.lin.bind(args, self.dbuf.data_ptr(), inputs)
        self.lout.bind(args, self.obuf.data_ptr(), outputs)

    def device_in(self, name):
        return _device_view(self.lin, self.dbuf, name)

    def device_out(self, name):
        return _device_view(self.lout, self.obuf, name)

    def workspace_bytes(self, export, args):
        nbytes = int(getattr(self.lib, export)(C.byref(args)))
        if nbytes == 0:
            raise _lib.StError(f'{export}: invalid sizes')
        return nbytes

    def workspace(self, args, nbytes):
        self.ws = torch.empty(nbytes, dtype=torch.uint8, device=self.dev)
        args.ws, args.ws_bytes = C.c_void_p(self.ws.data_ptr()), nbytes

    @contextlib.contextmanager
    def stages(self):
        """The launches go inside: the call's device is current, the stream is its current stream."""
        with torch.cuda.device(self.dev):
            self.stream = _lib.current_stream()
            yield
            self.begin(None)

    def begin(self, name):
        """A named interval of stages_ms begins here (launch() begins one where the export's name changes)."""
        if self.timing:
            event = torch.cuda.Event(enable_timing=True)
            event.record()
            self.events.append((name, event))
        self.interval = name

    def launch(self, name, *cargs, ok=(0,)):
        """lib.<name>(*cargs, stream), counted and checked; returns the code, which `ok` may allow to be another."""
        if name != self.interval:
            self.begin(name)
        self.launches[name] += 1
        rc = getattr(self.lib, name)(*cargs, self.stream)
        if rc not in ok:
            _lib.check(rc, name)
        return rc

    def fetch(self):
        """The one wait and the one copy back: the outputs as host views, by name."""
        host = self.obuf.cpu().numpy()
        self.t_back = time.perf_counter()
        return {k: self.lout.view(host, k) for k in self.lout.items}

    def timing_dict(self, **extra):
        t_end = time.perf_counter()
        ev = self.events
        return dict(extra, stages_ms={ev[i][0]: ev[i][1].elapsed_time(ev[i + 1][1]) for i in range(len(ev) - 1)},
                    host_prepare_s=self.t_prep - self.t_start, device_and_copies_s=self.t_back - self.t_prep,
                    host_finish_s=t_end - self.t_back, total_s=t_end - self.t_start)
