"""Base of the token-reduction methods, with the surface of llmc's TokenReductionModule
(llmc/compression/token_reduction/token_reduction_module.py:7-34): it reads what the model adapter knows about its vision tokens
(`model.pruning_config`) into the method's `special` section."""


class TokenReductionModule:
    def __init__(self, config, model, blocks):
        self.config = config
        self.model = model
        self.blocks = blocks
        self.set_sparse_config()

    def set_sparse_config(self):
        self.special_config = self.config.get('special', {})
        self.special_config['is_video_model'] = self.model.pruning_config['is_video_model']
        # vision_token can be image or video
        kind = 'video' if self.special_config['is_video_model'] else 'image'
        # .get: an adapter that leaves the index out lets the method take it from the model's own package (divprune.py)
        self.special_config['vision_token_index'] = self.model.pruning_config.get(f'{kind}_token_index')
        self.special_config['vision_token_length'] = self.model.pruning_config[f'{kind}_token_length']

    def register_reduction_modules(self):
        pass
