"""reagent/evaluation: what of the reference's evaluation package exists here -- offline evaluation of contextual bandits."""
