"""What the encoder modules share on the host side: one cache of the packed eval engine and one of the trainer handle."""


class EngineHost:
    """Mixin of the encoder nn.Modules: `_engine_cls` / `_trainer_cls` name the classes of `..engine`, `_anchor` the parameter whose device
    is the encoder's.  The module provides `cfg` and `numerics`."""
    _engine_cls = _trainer_cls = None
    _anchor = 'pos_embed'
    _engine = _engine_key = _trainer = None

    def _device(self, what):
        dev = getattr(self, self._anchor).device
        if dev.type != 'cuda':
            raise RuntimeError('fsvit: the encoder lives on %s; the HIP %s needs an MI355X (no CPU fallback)' % (dev, what))
        return dev

    def engine(self):
        """Packed HIP engine for the current weights (re-packed when any tensor changed)."""
        from .. import engine as E
        dev = self._device('engine')
        key = (E.weights_fingerprint(self), self.numerics, str(dev))
        if self._engine is None or self._engine_key != key:
            self._engine = getattr(E, self._engine_cls)(self.cfg, self.state_dict(), numerics=self.numerics, device=dev)
            self._engine_key = key
        return self._engine

    def trainer(self):
        from .. import engine as E
        dev = self._device('trainer')
        if self._trainer is None or self._trainer.device != dev:
            self._trainer = getattr(E, self._trainer_cls)(self.cfg, numerics=self.numerics, device=dev)
        return self._trainer
